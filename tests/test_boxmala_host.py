"""The numpy restatement of the MALA step kernel (tests/boxmala_ref.py, DESIGN I.19) against posteriors known in closed form,
and the reversibility identity of one step.  No device.

A statistical comparison here is a z-score: (the chains' average of a quantity - its exact expectation) / its standard error,
the standard error from the chains' own effective sample size (calibrate.ess of that quantity's series).  The margin is 5."""
import numpy as np
import pytest

import boxmala_ref as M

MARGIN = 5.0


def gain(w):
    from dgp_amd import calibrate
    return calibrate.gain(w, 0.574)


def zscore(series, exact):
    """series (R, S): a quantity along R chains."""
    from dgp_amd import calibrate
    series = np.asarray(series)
    return float((series.mean() - exact) / (series.std() / np.sqrt(calibrate.ess(series))))


def run_chains(fun, x0, w, ybar, lo, hi, s, seed, warmup, S, pv=None, pm=None):
    """R chains on calibrate's schedule and calibrate's streams (P = 1): samples (R, S, D), the chains."""
    from dgp_amd import calibrate
    R, D = x0.shape
    z, logu = calibrate.Streams(seed, 1, R, D).block(1 + warmup + S)
    chains = [M.sample(fun, x0[r], w, ybar, lo, hi, s, z[:, 0, r], logu[:, 0, r], warmup, 1, gain, pv, pm) for r in range(R)]
    return np.array([c.xs for c in chains]), chains


@pytest.mark.parametrize('D', [1, 2, 5])
def test_gaussian_posterior_well_inside_the_box(D):
    """f(x) = A x, K = D + 1 outputs, a flat prior on a box 40 posterior standard deviations wide: the posterior is
    N(mu, Sigma), Sigma = (A^T W A)^-1, mu = Sigma A^T W ybar.  4 chains of 3000 samples after 500 warm-up rounds; every
    mean, variance and covariance within 5 standard errors.  Observed (seed 11 + D), largest |z| over the means and over
    the second moments: D = 1: 1.28, 0.74; D = 2: 1.50, 1.28; D = 5: 0.55, 1.85."""
    rng = np.random.default_rng(100 + D)
    K = D + 1
    A = rng.normal(size=(K, D))
    w = rng.uniform(50.0, 200.0, K)
    ybar = A @ rng.uniform(-0.2, 0.2, D) + rng.normal(size=K) / np.sqrt(w)
    Sigma = np.linalg.inv(A.T @ (w[:, None] * A))
    mu = Sigma @ A.T @ (w * ybar)
    half = 20.0 * np.sqrt(np.diag(Sigma)).max() + np.abs(mu).max()
    lo, hi = np.full(D, -half), np.full(D, half)
    x0 = mu + rng.normal(size=(4, D)) * np.sqrt(np.diag(Sigma))
    xs, chains = run_chains(lambda x: (A @ x, A), x0, w, ybar, lo, hi, hi - lo, 11 + D, 500, 3000)
    assert all(c.status == M.OK and c.n_prop == 3500 for c in chains)
    zm = [zscore(xs[:, :, d], mu[d]) for d in range(D)]
    zc = [zscore((xs[:, :, a] - mu[a]) * (xs[:, :, b] - mu[b]), Sigma[a, b]) for a in range(D) for b in range(a, D)]
    print('D %d: acceptance %s, z of the means %s, of the second moments %s' %
          (D, np.round([c.n_acc / c.n_prop for c in chains], 2), np.round(zm, 2), np.round(zc, 2)))
    assert np.max(np.abs(zm)) <= MARGIN and np.max(np.abs(zc)) <= MARGIN


def test_truncated_normal_with_an_active_bound():
    """f(x) = x, ybar = 0.9, sd 0.3 on [0, 1]: a normal truncated at 1, a third of a standard deviation above its mode.
    Mean and variance against scipy.stats.truncnorm.  Observed z (seed 5): mean 2.03, variance -0.77."""
    from scipy.stats import truncnorm
    m, sd = 0.9, 0.3
    exact = truncnorm((0.0 - m) / sd, (1.0 - m) / sd, loc=m, scale=sd)
    lo, hi = np.zeros(1), np.ones(1)
    x0 = np.array([[0.2], [0.5], [0.8], [0.95]])
    xs, chains = run_chains(lambda x: (x.copy(), np.eye(1)), x0, np.array([1.0 / sd ** 2]), np.array([m]), lo, hi, hi - lo, 5, 500, 4000)
    assert xs.min() >= 0.0 and xs.max() <= 1.0
    zm, zv = zscore(xs[:, :, 0], exact.mean()), zscore((xs[:, :, 0] - exact.mean()) ** 2, exact.var())
    print('truncated normal: z of the mean %.2f, of the variance %.2f' % (zm, zv))
    assert abs(zm) <= MARGIN and abs(zv) <= MARGIN


def test_flat_likelihood_gives_the_uniform_distribution():
    """w = 0 (the one output is unobserved: its value and Jacobian hold NaN and are not read) and no prior: the samples
    are uniform on the box, mean (lo + hi) / 2 and variance (hi - lo)^2 / 12.  Observed z (seed 9): means -0.17, -0.64;
    variances -0.85, -0.55."""
    lo, hi = np.array([-1.0, 0.0]), np.array([2.0, 1.0])
    x0 = np.random.default_rng(3).uniform(lo, hi, (4, 2))
    nan = lambda x: (np.full(1, np.nan), np.full((1, 2), np.nan))
    xs, chains = run_chains(nan, x0, np.zeros(1), np.full(1, np.nan), lo, hi, hi - lo, 9, 500, 4000)
    assert all(c.status == M.OK for c in chains) and np.all(xs >= lo) and np.all(xs <= hi)
    mid, var = 0.5 * (lo + hi), (hi - lo) ** 2 / 12.0
    zm = [zscore(xs[:, :, d], mid[d]) for d in range(2)]
    zv = [zscore((xs[:, :, d] - mid[d]) ** 2, var[d]) for d in range(2)]
    print('uniform: z of the means %s, of the variances %s' % (np.round(zm, 2), np.round(zv, 2)))
    assert np.max(np.abs(zm)) <= MARGIN and np.max(np.abs(zv)) <= MARGIN


def reversal(step_fn, D=3, K=2, seed=0):
    """One step x -> x' with noise z, then from a fresh state at x' the step with the noise that maps back: (the two
    stored log ratios, the bound on their sum).  step_fn(x0, z, fun, ...) -> (trial, logr) runs INIT and one decision.
    The bound: the second step lands on x up to the rounding of x' + c g' + h s z', a few ulps of |x| + |x'| per column;
    that moves u and v by that over h s and lp by |g| times it, and every sum adds its own roundings: 16 eps times
    |lp| + |lp'| + qf + qb + sum_d (|u_d| + |v_d| + |g_d| + |g'_d|) (|x_d| + |x'_d|) / (h s_d) is first-order safe."""
    rng = np.random.default_rng(seed)
    a, b = rng.normal(size=(K, D)), rng.normal(size=K)
    fun = lambda x: (np.sin(a @ x + b), np.cos(a @ x + b)[:, None] * a)
    w, ybar, lo, hi, s, h = rng.uniform(1.0, 4.0, K), rng.normal(size=K), np.full(D, -5.0), np.full(D, 5.0), rng.uniform(0.5, 2.0, D), 0.3
    x, z = rng.uniform(-1.0, 1.0, D), rng.normal(size=D)
    args = (w, ybar, lo, hi, s)
    x1, r1 = step_fn(x, z, fun, args, h)
    ref = M.Chain(x, *args, h0=h)
    lp, g = ref.target(x, *fun(x))
    lp1, g1 = ref.target(x1, *fun(x1))
    c, hs = 0.5 * h * h * s * s, h * s
    back = (x - x1 - c * g1) / hs
    x2, r2 = step_fn(x1, back, fun, args, h)
    u, v = (x1 - x - c * g) / hs, (x - x1 - c * g1) / hs
    size = abs(lp) + abs(lp1) + u @ u + v @ v + np.sum((np.abs(u) + np.abs(v) + np.abs(g) + np.abs(g1)) * (np.abs(x) + np.abs(x1)) / hs)
    assert np.max(np.abs(x2 - x)) <= 8 * np.finfo(float).eps * np.max(np.abs(x) + np.abs(x1))
    return r1, r2, 16 * np.finfo(float).eps * size


def ref_step(x, z, fun, args, h):
    ch = M.Chain(x, *args, h0=h)
    ch.step(*fun(ch.trial), z, 0.0)
    trial = ch.trial.copy()
    ch.step(*fun(ch.trial), np.zeros(len(x)), 0.0)
    return trial, ch.logr


@pytest.mark.parametrize('seed', range(5))
def test_reversibility_exactly(seed):
    r1, r2, bound = reversal(ref_step, seed=seed)
    print('log ratios %.17g, %.17g: sum %.3g, bound %.3g' % (r1, r2, r1 + r2, bound))
    assert np.isfinite(r1) and r1 != 0.0 and abs(r1 + r2) <= bound


def test_the_restatements_edge_cases():
    """A start that is not finite: status NAN, the trial and every saved sample stay the start.  A proposal thrown out of
    the box: rejected, and the point evaluated in between is x.  A fixed column and a column with s = 0 never move."""
    lo, hi, s = np.array([0.0, 0.0, 0.3]), np.array([1.0, 1.0, 0.3]), np.array([1.0, 0.0, 1.0])
    fun = lambda x: (x[:1].copy(), np.array([[1.0, 0.0, 0.0]]))
    x0 = np.array([0.5, 0.25, 0.3])
    bad = M.Chain(x0, np.ones(1), np.zeros(1), lo, hi, s)
    bad.step(np.full(1, np.nan), fun(x0)[1], np.zeros(3), 0.0, save=True)
    bad.step(*fun(bad.trial), np.ones(3), -np.inf, save=True)
    assert bad.status == M.NAN and bad.n_prop == 0 and np.array_equal(bad.trial, x0) and np.array_equal(bad.xs, [x0, x0])
    ch = M.Chain(x0, np.ones(1), np.zeros(1), lo, hi, s)
    ch.step(*fun(ch.trial), np.array([1e6, 1.0, 1.0]), 0.0)
    assert ch.flag and np.array_equal(ch.trial, x0)
    ch.step(*fun(ch.trial), np.array([0.1, 1.0, 1.0]), -np.inf)
    assert ch.logr == -np.inf and ch.n_prop == 1 and ch.n_acc == 0 and not ch.flag
    assert ch.trial[0] != x0[0] and np.array_equal(ch.trial[1:], x0[1:])
    ch.step(*fun(ch.trial), np.zeros(3), -np.inf)
    assert ch.n_acc == 1 and np.array_equal(ch.x[1:], x0[1:])


def test_status_numbers_and_workspace_match_the_header():
    """Engine.BOXMALA carries the header's DGPAMD_BOXMALA_* numbers, all of them, and the restatement's; the workspace is
    x, g, g' and lp as doubles and one int32 flag per chain (a host-side formula: no device)."""
    import os
    import re
    from dgp_amd import _lib
    from dgp_amd.ops import Engine
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, 'include', 'dgp_amd.h')).read()
    header = {k.lower(): int(v) for k, v in re.findall(r'#define\s+DGPAMD_BOXMALA_([A-Z]+)\s+(\d+)', src)}
    count = header.pop('count')
    assert header == Engine.BOXMALA and sorted(header.values()) == list(range(count))
    assert (Engine.BOXMALA['ok'], Engine.BOXMALA['nan']) == (M.OK, M.NAN)
    for Q, D in ((1, 1), (130, 5), (800, 64)):
        assert Engine.boxmala_workspace(Q, D) == Q * (8 * (3 * D + 1) + 4)
    for Q, D in ((0, 5), (4, 0), (4, 65), (1 << 31, 5)):
        with pytest.raises(ValueError):
            Engine.boxmala_workspace(Q, D)
    # the other host-side checks are exercised by tools/boxchain_args_check.cpp under the sanitizers
    assert _lib.lib.dgpamd_boxmala_step(None, 1, 1, 1, *[None] * 6, 0.1, 1e-10, 1e2, 1.0, 1.0, 0, 1, -1, 0, *[None] * 9) == _lib.BAD_ARG
