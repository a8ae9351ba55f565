"""Field calibration on the host (dgp_amd/fieldcal.py, tests/boxsites_ref.py, DESIGN I.24): the whitening against plain
algebra on the covariance, the fold's restatement against its scalar form, posteriors known in closed form sampled by the numpy
restatements of the chain kernels on the fold's output, and every refusal of the data model.  No device.

A statistical comparison is test_boxmala_host's z-score, the standard error from the chains' own effective sample size, margin 5."""
import numpy as np
import pytest

import boxhmc_ref as HM
import boxmala_ref as M
import boxsites_ref as B
import test_boxmala_host as H

MARGIN = H.MARGIN
EPS = np.finfo(float).eps


def whiteners():
    from dgp_amd import fieldcal
    return {'fieldcal': lambda y, sd, cov: fieldcal.whiten(y, sd, cov, np.shape(y)[1]), 'ref': B.whiten}


def messy_case(seed=0, T=7, K=2):
    """y (T, K) with two NaN entries, obs_sd (T, K), obs_cov (K, T, T) of squared-exponential form: cond(Sigma_k) <= 40."""
    rng = np.random.default_rng(seed)
    c = np.sort(rng.uniform(0.0, 1.0, T))
    cov = np.array([a * a * np.exp(-(c[:, None] - c[None]) ** 2 / (2.0 * l * l)) for a, l in ((0.1, 0.3), (0.2, 0.15))][:K])
    sd = rng.uniform(0.05, 0.1, (T, K))
    y = rng.normal(size=(T, K))
    y[2, 0] = y[5, K - 1] = np.nan
    return y, sd, cov


@pytest.mark.parametrize('which', ['fieldcal', 'ref'])
def test_whitening_is_the_quadratic_form(which):
    """sum_j w_j (ybar_j - ft_j)^2 = sum_k r_k^T Sigma_k^-1 r_k within 64 T cond(Sigma) eps relative: the triangular solve and the
    products each lose a few T cond eps.  The matrices: the line case (cond 12.5: observed relative difference 0 against the
    bound 8.9e-13) and messy_case (cond 14.3, T = 7, NaN entries: 5.4e-16 against 1.4e-12).  log_norm + -1/2 the form is the multivariate normal's logpdf
    over the observed entries."""
    from scipy.stats import multivariate_normal
    white = whiteners()[which]
    c, sd, cov, Sigma = B.line_case()
    assert abs(np.linalg.cond(Sigma) - 12.5) < 0.05
    rng = np.random.default_rng(1)
    cases = [(rng.normal(size=(5, 1)), sd, cov), messy_case()]
    for y, sd, cov in cases:
        T, K = y.shape
        W, ybar, w, log_norm = white(y, sd, cov)
        Sig = B.covariances(T, K, sd, cov)
        cond = max(np.linalg.cond(S) for S in Sig)
        f = rng.normal(size=(1, T, K))
        ft = B.fold(np.where(np.isnan(y), np.nan, f), None, W, [])[0][0]           # (an unobserved site's value is NaN: not read)
        got = np.sum(w * (ybar - ft) ** 2)
        want = B.quadratic_form(y - f[0], Sig)
        print('%s T %d K %d cond %.1f: relative difference %.2g, bound %.2g' % (which, T, K, cond, abs(got - want) / want, 64 * T * cond * EPS))
        assert abs(got - want) <= 64 * T * cond * EPS * want
        logpdf = 0.0
        for k in range(K):
            at = np.nonzero(~np.isnan(y[:, k]))[0]
            logpdf += multivariate_normal.logpdf(y[at, k], f[0, at, k], Sig[k][np.ix_(at, at)])
        assert abs(log_norm - 0.5 * got - logpdf) <= 64 * T * cond * EPS * abs(logpdf) + 1e-13
        assert np.array_equal(W, np.tril(W)) and set(np.unique(w)) <= {0.0, 1.0}


@pytest.mark.parametrize('which', ['fieldcal', 'ref'])
def test_unobserved_entries_drop_out(which):
    """Marginalising a Gaussian deletes rows and columns: with NaN at sites 1 and 4 the whitened problem is that of the other
    sites alone, bit for bit, and W's rows and columns of the two are exactly zero."""
    white = whiteners()[which]
    c, sd, cov, _ = B.line_case()
    y = np.random.default_rng(2).normal(size=(5, 1))
    gone, kept = [1, 4], [0, 2, 3]
    y_nan = y.copy()
    y_nan[gone] = np.nan
    W, ybar, w, ln = white(y_nan, sd, cov)
    W2, ybar2, w2, ln2 = white(y[kept], sd, cov[np.ix_(kept, kept)])
    assert np.all(W[0][gone] == 0.0) and np.all(W[0][:, gone] == 0.0) and np.all(ybar[gone] == 0.0)
    assert np.array_equal(w, [1.0, 0.0, 1.0, 1.0, 0.0]) and np.all(w2 == 1.0)
    assert np.array_equal(W[0][np.ix_(kept, kept)], W2[0]) and np.array_equal(ybar[kept], ybar2) and ln == ln2
    # an output without any observation contributes nothing; obs_sd per entry is used where the entry is
    y2 = np.column_stack([y_nan[:, 0], np.full(5, np.nan)])
    W3, ybar3, w3, ln3 = white(y2, np.column_stack([np.full(5, sd), np.full(5, 7.0)]), cov)
    assert np.array_equal(W3[0], W[0]) and np.all(W3[1] == 0.0) and ln3 == ln and np.array_equal(w3.reshape(5, 2)[:, 0], w)


def test_the_two_whitenings_agree_and_the_diagonal_is_one_over_sd():
    from dgp_amd import fieldcal
    y, sd, cov = messy_case()
    a, b = fieldcal.whiten(y, sd, cov, 2), B.whiten(y, sd, cov)
    for u, v in zip(a, b):
        assert np.allclose(u, v, rtol=1e-12, atol=1e-13)
    W, ybar, w, ln = fieldcal.whiten(y, sd, None, 2)
    seen = ~np.isnan(y)
    for k in range(2):
        assert np.array_equal(W[k], np.diag(np.where(seen[:, k], 1.0 / sd[:, k], 0.0)))
    assert np.array_equal(ybar.reshape(7, 2), np.where(seen, y, 0.0) * np.where(seen, 1.0 / sd, 0.0))
    assert np.isclose(ln, -0.5 * seen.sum() * np.log(2 * np.pi) - np.log(sd[seen]).sum(), rtol=1e-14)
    # T = 1 with a scalar sd is calibrate's own observation: w = 1 / sd^2 on (y - f) against 1 on (y / sd - f / sd)
    W1, yb1, w1, _ = fieldcal.whiten(np.array([[0.3, np.nan, -1.0]]), 0.25, None, 3)
    assert np.array_equal(W1[:, 0, 0], [4.0, 0.0, 4.0]) and np.array_equal(yb1, [1.2, 0.0, -4.0]) and np.array_equal(w1, [1.0, 0.0, 1.0])


@pytest.mark.parametrize('T,K,Dx,cols', [(1, 1, 2, [1]), (4, 2, 3, [2, 0]), (7, 3, 5, [4, 1, 3])])
def test_fold_equals_its_scalar_form(T, K, Dx, cols):
    """The vectorised restatement against the header's text as loops, array_equal: a dense W, a diagonal W, and sites 1 and T - 2
    unobserved with NaN in their f and J (outputs there 0, no NaN anywhere else)."""
    rng = np.random.default_rng(T)
    f, J = rng.normal(size=(3, T, K)), rng.normal(size=(3, T, K, Dx))
    dense = np.tril(rng.normal(size=(K, T, T)))
    for W in (dense, dense * np.eye(T)):
        got, want = B.fold(f, J, W, cols), B.fold_scalar(f, J, W, cols)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert np.array_equal(B.fold(f, None, W, [])[0], want[0])
    if T >= 4:
        gone = [1, T - 2]
        W = dense.copy()
        W[:, gone], W[:, :, gone] = 0.0, 0.0
        f[:, gone], J[:, gone] = np.nan, np.nan
        got, want = B.fold(f, J, W, cols), B.fold_scalar(f, J, W, cols)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert np.all(np.isfinite(got[0])) and np.all(np.isfinite(got[1]))
        assert np.all(got[0].reshape(3, T, K)[:, gone] == 0.0) and np.all(got[1].reshape(3, T, K, -1)[:, gone] == 0.0)


# ---------------------------------------------------------------------------------------------------- closed-form posteriors
def line_problem(seed=3):
    """The line case with data: theta = 0.7, the errors drawn from Sigma.  The walk's input is (c, theta): column 0 the control,
    column 1 calibrated.  Returns (y (5, 1), fun(theta (1,)) -> the fold's (ft (5,), Jt (5, 1)), W, ybar, w, Sigma, c)."""
    c, sd, cov, Sigma = B.line_case()
    y = (0.7 * c + np.linalg.cholesky(Sigma) @ np.random.default_rng(seed).normal(size=5))[:, None]
    W, ybar, w, _ = B.whiten(y, sd, cov)

    def fun(theta):
        f = (theta[0] * c)[None, :, None]
        J = np.stack([np.full(5, theta[0]), c], -1)[None, :, None, :]           # d f / d (c, theta)
        ft, Jt = B.fold(f, J, W, [1])
        return ft[0], Jt[0]
    return y, fun, W, ybar, w, Sigma, c


def test_correlation_changes_the_closed_form():
    """Exact algebra on the whitened problem: the posterior of theta under a flat prior is N(A^T ybar / A^T A, 1 / A^T A) with
    A = W c.  Its sd is 0.10632 (and equals 1 / sqrt(c^T Sigma^-1 c) by np.linalg.solve); with the diagonal of Sigma alone it is
    0.07538; the variances differ by the factor 1.990."""
    y, fun, W, ybar, w, Sigma, c = line_problem()
    A = W[0] @ c
    sd_full = 1.0 / np.sqrt(A @ A)
    assert abs(sd_full - 0.10632) < 5e-6 and abs(sd_full * np.sqrt(c @ np.linalg.solve(Sigma, c)) - 1.0) < 64 * 5 * 12.5 * EPS
    Wd = B.whiten(y, np.sqrt(np.diag(Sigma))[:, None], None)[0]
    Ad = Wd[0] @ c
    sd_diag = 1.0 / np.sqrt(Ad @ Ad)
    assert abs(sd_diag - 0.07538) < 5e-6 and abs((sd_full / sd_diag) ** 2 - 1.990) < 5e-4
    mean = A @ ybar / (A @ A)
    assert abs(mean - c @ np.linalg.solve(Sigma, y[:, 0]) / (c @ np.linalg.solve(Sigma, c))) < 1e-12
    # the fold's Jacobian of the calibrated column is A itself
    ft, Jt = fun(np.array([0.4]))
    assert np.allclose(Jt[:, 0], A, rtol=1e-15, atol=0) and np.allclose(ft, 0.4 * A, rtol=4 * EPS, atol=0)


def line_moments(xs, y, W, ybar, Sigma, c):
    A = W[0] @ c
    var = 1.0 / (A @ A)
    mean = var * (A @ ybar)
    var_diag = 1.0 / np.sum(c * c / np.diag(Sigma))
    th = xs[:, :, 0]
    return (H.zscore(th, mean), H.zscore((th - mean) ** 2, var), H.zscore((th - mean) ** 2, var_diag))


def test_mala_samples_the_correlated_posterior():
    """boxmala_ref.Chain on fold's output, 4 chains of 3000 samples after 500 warm-up rounds on calibrate's streams, a flat
    prior on [-2, 3] (25 posterior standard deviations to either wall): mean and variance within 5 standard errors by the
    chains' own ess.  The margin rejects the diagonal-only answer by construction -- its variance is 1.99 times smaller, so
    the same samples lie many standard errors from it, which is asserted too.
    Observed (seed 21): z of the mean -0.57, of the variance 0.52; against the diagonal-only variance 19.2."""
    y, fun, W, ybar, w, Sigma, c = line_problem()
    lo, hi = np.array([-2.0]), np.array([3.0])
    x0 = np.array([[0.2], [0.6], [0.9], [1.3]])
    xs, chains = H.run_chains(fun, x0, w, ybar, lo, hi, hi - lo, 21, 500, 3000)
    assert all(ch.status == M.OK for ch in chains)
    zm, zv, zd = line_moments(xs, y, W, ybar, Sigma, c)
    print('mala: z of the mean %.2f, of the variance %.2f; against the diagonal-only variance %.2f' % (zm, zv, zd))
    assert abs(zm) <= MARGIN and abs(zv) <= MARGIN and zd > MARGIN


def test_hmc_samples_the_correlated_posterior():
    """The same with boxhmc_ref's chain: calibrate's HMC schedule, n_leapfrog 8 with jitter, target 0.8.
    Observed (seed 22): z of the mean -1.23, of the variance -0.24; against the diagonal-only variance 17.8."""
    from dgp_amd import calibrate
    y, fun, W, ybar, w, Sigma, c = line_problem()
    lo, hi = np.array([-2.0]), np.array([3.0])
    x0 = np.array([[0.2], [0.6], [0.9], [1.3]])
    warmup, S, seed = 300, 2000, 22
    z, logu = calibrate.Streams(seed, 1, 4, 1).block(1 + warmup + S)
    lengths = calibrate.trajectory_lengths(seed, warmup + S, 8, True)
    gain = lambda i: calibrate.gain(i, 0.8)
    chains = [HM.sample(fun, x0[r], w, ybar, lo, hi, hi - lo, z[:, 0, r], logu[:, 0, r], lengths, warmup, 1, gain) for r in range(4)]
    assert all(ch.status == HM.OK for ch in chains)
    zm, zv, zd = line_moments(np.array([ch.xs for ch in chains]), y, W, ybar, Sigma, c)
    print('hmc: z of the mean %.2f, of the variance %.2f; against the diagonal-only variance %.2f' % (zm, zv, zd))
    assert abs(zm) <= MARGIN and abs(zv) <= MARGIN and zd > MARGIN


def test_two_parameters_two_outputs_one_entry_unobserved():
    """f_k(c, theta) = theta_0 a_k(c) + theta_1 b_k(c), K = 2 outputs at T = 6 sites, entry (3, 1) unobserved, each output its
    own covariance: the posterior under a flat prior is the generalised-least-squares one, covariance (sum_k X_k^T Sigma_k^-1
    X_k)^-1 over the observed rows, by np.linalg.solve.  The walk's input is (theta_0, c, theta_1): the calibrated columns 0
    and 2 are not contiguous.  MALA under the same rule.  Observed (seed 23), largest |z|: means 1.24, second moments 0.17."""
    rng = np.random.default_rng(5)
    T, K = 6, 2
    c = np.linspace(0.0, 1.0, T)
    X = np.stack([np.stack([np.ones(T), c], 1), np.stack([np.sin(2.0 * c), c * c], 1)])       # (K, T, 2): a_k, b_k
    dX = np.stack([np.stack([np.zeros(T), np.ones(T)], 1), np.stack([2.0 * np.cos(2.0 * c), 2.0 * c], 1)])   # d a_k / dc, d b_k / dc
    cov = np.array([s * s * np.exp(-(c[:, None] - c[None]) ** 2 / (2.0 * l * l)) for s, l in ((0.1, 0.3), (0.15, 0.5))])
    sd = np.array([0.05, 0.08])
    Sigma = B.covariances(T, K, sd, cov)
    truth = np.array([0.5, -0.3])
    y = np.stack([X[k] @ truth + np.linalg.cholesky(Sigma[k]) @ rng.normal(size=T) for k in range(K)], 1)
    y[3, 1] = np.nan
    W, ybar, w, _ = B.whiten(y, sd, cov)

    def fun(theta):
        f = np.stack([X[k] @ theta for k in range(K)], 1)                                       # (T, K)
        J = np.stack([np.stack([X[k][:, 0], dX[k] @ theta, X[k][:, 1]], 1) for k in range(K)], 1)   # (T, K, 3)
        f[3, 1], J[3, 1] = np.nan, np.nan
        ft, Jt = B.fold(f[None], J[None], W, [0, 2])
        return ft[0], Jt[0]
    prec, rhs = np.zeros((2, 2)), np.zeros(2)
    for k in range(K):
        at = np.nonzero(~np.isnan(y[:, k]))[0]
        S = Sigma[k][np.ix_(at, at)]
        prec += X[k][at].T @ np.linalg.solve(S, X[k][at])
        rhs += X[k][at].T @ np.linalg.solve(S, y[at, k])
    Cov = np.linalg.inv(prec)
    mu = Cov @ rhs
    half = 20.0 * np.sqrt(np.diag(Cov)).max() + np.abs(mu).max()
    lo, hi = np.full(2, -half), np.full(2, half)
    x0 = mu + rng.normal(size=(4, 2)) * np.sqrt(np.diag(Cov))
    xs, chains = H.run_chains(fun, x0, w, ybar, lo, hi, hi - lo, 23, 500, 3000)
    assert all(ch.status == M.OK for ch in chains)
    zm = [H.zscore(xs[:, :, d], mu[d]) for d in range(2)]
    zc = [H.zscore((xs[:, :, a] - mu[a]) * (xs[:, :, b] - mu[b]), Cov[a, b]) for a in range(2) for b in range(a, 2)]
    print('gls: z of the means %s, of the second moments %s' % (np.round(zm, 2), np.round(zc, 2)))
    assert np.max(np.abs(zm)) <= MARGIN and np.max(np.abs(zc)) <= MARGIN
    # the chains' log density is the field log posterior up to rounding
    th = xs[0, -1]
    f = np.stack([X[k] @ th for k in range(K)], 1)
    assert abs(chains[0].lps[-1] - B.field_logp(y, f, sd, cov)) <= 64 * T * 40 * EPS * abs(chains[0].lps[-1])


# ------------------------------------------------------------------------------------------------------------------ refusals
def fake_lane(K=2, read=2):
    """A container's _lane_problem without a device: K outputs, the model reads columns 0 .. read."""
    def lane(bounds, what):
        Dx = np.asarray(bounds).shape[0]
        if Dx <= read:
            raise ValueError('%s: bounds has %d rows, the emulator reads column %d of its input' % (what, Dx, read))
        return None, 3, K, Dx, None, None, 10
    return lane


def test_every_refusal_of_the_data_model():
    from dgp_amd import fieldcal
    T, K = 4, 2
    good = dict(y=np.zeros((T, K)), obs_sd=0.1, bounds=[[0.0, 1.0], [0.0, 1.0]], controls=np.linspace(0, 1, T)[:, None],
                control_columns=[1], obs_cov=0.01 * np.eye(T))

    def refused(match=None, lane=fake_lane(K), **change):
        kw = dict(good, **change)
        with pytest.raises(ValueError, match=match):
            fieldcal.prepare(lane, 'calibrate', kw['y'], kw['obs_sd'], kw['bounds'], kw['controls'], kw['control_columns'], kw['obs_cov'])
    # without controls: obs_cov and control_columns mean nothing; the old path is the lane's own tuple and no problem
    refused('need controls', controls=None, control_columns=None)
    refused('need controls', controls=None, obs_cov=None)
    lane, problem = fieldcal.prepare(fake_lane(K), 'calibrate', good['y'], 0.1, np.zeros((3, 2)), None, None, None)
    assert problem is None and lane[3] == 3
    # controls
    refused('controls must be', controls=np.zeros(T))
    refused('controls must be', controls=np.zeros((0, 1)))
    refused('controls must be', controls=np.zeros((T, 0)))
    refused('controls must be', controls=np.full((T, 1), np.nan))
    refused('controls must be', controls=np.zeros((fieldcal.MAX_SITES + 1, 1)), y=np.zeros((fieldcal.MAX_SITES + 1, K)), obs_cov=None)
    # control_columns
    refused('control_columns', control_columns=None)
    refused('control_columns', control_columns=[0, 1])
    refused('control_columns', control_columns=[0.5])
    refused('control_columns', controls=np.zeros((T, 2)), control_columns=[1, 1])
    refused('control_columns', control_columns=[3])
    refused('control_columns', control_columns=[-1])
    # the calibration columns: at least 1, at most 64, and with the controls every column the model reads
    refused('bounds', bounds=np.zeros((0, 2)))
    refused('bounds', bounds=np.zeros((65, 2)))
    refused('bounds', bounds=[0.0, 1.0])
    refused('reads column', bounds=[[0.0, 1.0]])
    # y, obs_sd
    refused('y must be', y=np.zeros((T, K + 1)))
    refused('y must be', y=np.zeros(T))
    refused('y must be finite', y=np.full((T, K), np.inf))
    refused('no finite entry', y=np.full((T, K), np.nan))
    refused('rows', y=np.zeros((T + 1, K)), obs_cov=None)
    for sd in (0.0, -1.0, np.nan, np.zeros(K), np.ones(T), np.ones((K, T)), np.full((T, K), np.inf)):
        refused('obs_sd', obs_sd=sd)
    # obs_cov: the shape, symmetry, and a covariance that does not factor
    refused('obs_cov must be', obs_cov=np.eye(T + 1))
    refused('obs_cov must be', obs_cov=np.zeros((K + 1, T, T)))
    refused('obs_cov must be', obs_cov=np.full((T, T), np.nan))
    refused('symmetric', obs_cov=np.triu(np.ones((T, T))))
    refused('positive definite', obs_cov=-np.eye(T))
    refused('positive definite', obs_cov=np.array([[1.0, 2.0], [2.0, 1.0]]), y=np.zeros((2, K)), controls=np.zeros((2, 1)))
    # a 1-D y is one output's T values
    W, ybar, w, _ = fieldcal.whiten(np.arange(3.0), 0.5, None, 1)
    assert W.shape == (1, 3, 3) and np.array_equal(ybar, [0.0, 2.0, 4.0])


def test_the_results_carry_columns_and_controls():
    """The containers are calibrate's: PathPosterior and ParticlePosterior, columns and controls None unless the run had
    controls; the calibration columns are the others in increasing order."""
    from dgp_amd import calibrate, fieldcal
    assert calibrate.PathPosterior.columns is None and calibrate.PathPosterior.controls is None
    assert calibrate.ParticlePosterior.columns is None and calibrate.ParticlePosterior.controls is None
    c, cc, theta, Dx = fieldcal.check_controls(np.zeros((3, 2)), [4, 1], np.zeros((3, 2)), 'calibrate')
    assert Dx == 5 and np.array_equal(theta, [0, 2, 3]) and np.array_equal(cc, [4, 1]) and c.shape == (3, 2)
    import inspect
    from dgp_amd import pathfun
    for cls in (pathfun.PathFunctions, pathfun.GpPaths):
        for name in ('calibrate', 'calibrate_smc'):
            par = inspect.signature(getattr(cls, name)).parameters
            new = ['controls', 'control_columns', 'obs_cov']
            at = list(par).index('controls')
            # keyword-only, together, in front of the tail that tests/test_boxhmc_host.py and tests/test_philox_host.py pin
            assert list(par)[at:at + 3] == new and list(par)[at + 3:] == (['rng'] if name == 'calibrate_smc' else
                                                                          ['prior', 'rng', 'target_accept', 'method', 'n_leapfrog', 'jitter'])
            assert all(par[k].kind is inspect.Parameter.KEYWORD_ONLY and par[k].default is None for k in new)
            assert all(q.kind is not inspect.Parameter.KEYWORD_ONLY for q in list(par.values())[:at])


def test_the_header_and_the_engine_agree():
    import os
    import re
    from dgp_amd import _lib, fieldcal
    from dgp_amd.ops import Engine
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, 'include', 'dgp_amd.h')).read()
    assert int(re.search(r'#define\s+DGPAMD_BOXSITES_MAXT\s+(\d+)', src).group(1)) == Engine.BOXSITES_MAXT == fieldcal.MAX_SITES == 256
    # the other host-side checks are exercised by tools/boxsites_args_check.cpp under the sanitizers
    assert _lib.lib.dgpamd_boxsites_fold(None, 1, 1, 1, 1, 0, *[None] * 7) == _lib.BAD_ARG
