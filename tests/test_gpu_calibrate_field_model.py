"""paths.calibrate and paths.calibrate_smc with field data (dgp_amd/fieldcal.py, DESIGN I.24) on the small models of
tests/test_gpu_calibrate_model.py: known control inputs, a shared calibration parameter, errors correlated across the sites.
Every draw's posterior and evidence against quadrature on a grid of the draw's own whitened values, the log densities against
the field log posterior by np.linalg.solve, bit-for-bit replays and invariances, and the refusals.  Needs an MI355X: -m gpu.

The statistical bounds that are not z-scores come from the numpy restatements on the numpy replay of the same draws
(tests/test_fieldcal_host.py::test_field_case_on_the_cpu, which also holds the constants here to what it measures)."""
import types

import numpy as np
import pytest

import boxmala_ref as M
import boxsites_ref as S
import boxsmc_ref as SMC
import pathfun_ref as Rf
import pathgrad_ref as Rg
import test_boxmala_host as H
import test_gpu_boxmin_model as B
import test_gpu_pathfun as T

pytestmark = pytest.mark.gpu
MARGIN = 5.0
EPS = np.finfo(float).eps
# The field case: the 2-D gp on the bowl (x0 - 0.3)^2 + (x1 - 0.6)^2, column 0 the control at 5 sites, column 1 calibrated;
# Sigma = 0.05^2 I + 0.1^2 exp(-(c - c')^2 / (2 0.3^2)), cond 12.5.
FIELD = dict(J=6, F=128, seed=31, chains=4, samples=1000, warmup=500, particles=512, moves=4)
SITES, OBS_SD, OBS_COV, SIGMA = S.line_case()
Y = ((SITES - 0.3) ** 2)[:, None]          # (what the bowl gives at theta = 0.6: one flat-topped mode)
CONTROLS = SITES[:, None]
BOXT = np.array([[0.0, 1.0]])
GRID = np.linspace(0.0, 1.0, 4001)
FKW = dict(controls=CONTROLS, control_columns=[0], obs_cov=OBS_COV)
# The CPU run of the same case (test_field_case_on_the_cpu): split R-hat of the restatement's chains over the 6 draws, and over
# 16 seeds of boxsmc_ref the largest standard deviation of log_evidence over the draws.  RHAT_MAX is ten times the CPU run's
# largest distance from 1, the rule of test_gpu_calibrate_model.RHAT_MAX.
# Measured: MALA's split R-hat 0.9996 .. 1.0049, HMC's 0.9996 .. 1.0033; the spreads of log_evidence 0.0232 .. 0.0315.
CPU = dict(rhat_mala=1.0049, rhat_hmc=1.0033, field_logz=0.0315)
RHAT_MAX = dict(mala=1.0 + 10.0 * (CPU['rhat_mala'] - 1.0), hmc=1.0 + 10.0 * (CPU['rhat_hmc'] - 1.0))


@pytest.fixture(scope='module')
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    from dgp_amd.ops import default_engine
    return default_engine(0)


@pytest.fixture(scope='module')
def gp_paths(eng):
    X, Yb = B.bowl()
    m = T._gp('sexp', X, Yb)
    np.random.seed(FIELD['seed'])
    return m, m.sample_functions(sample_size=FIELD['J'], n_features=FIELD['F'])


def site_rows(theta):
    """theta (M,) -> the walk's rows (M T, 2), site fastest: (c_t, theta_m)."""
    return np.stack([np.tile(SITES, len(theta)), np.repeat(theta, len(SITES))], 1)


def bowl_case():
    """The fixed-hyperparameter gp on the bowl and its draws under np.random.seed(FIELD['seed']), in numpy: funs[p](theta (R, 1))
    -> the fold's (ft (R, 5), Jt (R, 5, 1)) of draw p through boxsites_ref, and the whitened draws on GRID (J, 4001, 5)."""
    X, Yb = B.bowl()
    kind, length, scale, nugget = 'sexp', np.full(2, 0.7), 1.9, 1e-4
    k = types.SimpleNamespace(name=kind, length=length, _X=lambda: X)
    _, Omega, b, theta, eps = T._gp_replay(types.SimpleNamespace(kernel=k), FIELD['seed'], FIELD['J'], FIELD['F'])
    v = Rf.weights(X, Yb[:, 0], Omega, b, theta, eps, kind, length, scale, nugget, None)
    W = S.whiten(Y, OBS_SD, OBS_COV)[0]

    def fun(th, p):
        x = site_rows(th[:, 0])
        f = Rf.evaluate(x, X, Omega, b, theta[p:p + 1], v[p:p + 1], kind, length, scale)[0].reshape(len(th), 5, 1)
        J = Rg.grad(x, X, Omega, b, theta[p:p + 1], v[p:p + 1], kind, length, scale)[0].reshape(len(th), 5, 1, 2)
        return S.fold(f, J, W, [1])
    funs = [lambda th, p=p: fun(th, p) for p in range(FIELD['J'])]
    f_grid = Rf.evaluate(site_rows(GRID), X, Omega, b, theta, v, kind, length, scale).reshape(FIELD['J'], len(GRID), 5, 1)
    return funs, np.array([S.fold(f, None, W, [])[0] for f in f_grid])


def whitened_grid(paths):
    """(W, ybar, w, log_norm, the device's own draws on GRID, whitened: (J, 4001, 5))."""
    W, ybar, w, log_norm = S.whiten(Y, OBS_SD, OBS_COV)
    f = paths(site_rows(GRID)).T.reshape(FIELD['J'], len(GRID), 5, 1)
    return W, ybar, w, log_norm, np.array([S.fold(fp, None, W, [])[0] for fp in f])


@pytest.mark.parametrize('method', ['mala', 'hmc'])
def test_field_gp_against_quadrature(eng, gp_paths, method):
    """6 draws x 4 chains x 1000 samples: per draw the mean and variance of theta within 5 standard errors, by the samples' own
    ess, of grid_posterior over the whitened paths(rows) on 4001 values of theta (the grid values are the device's own);
    split R-hat below the CPU run's bound.  Observed on an MI355X (seed 1): mala z of the means -0.14, 0.03, 0.71, 1.33, 0.75,
    2.29, of the variances 1.64, 1.40, 0.84, -1.87, -2.95, -0.94, split R-hat at most 1.0074, ess 451 .. 1747 of 4000,
    acceptance 0.47 .. 0.68; hmc z of the means 0.27, -1.14, 0.31, -0.17, -0.32, -0.57, of the variances 0.90, -0.58, 0.65,
    -0.02, 1.15, -0.59, split R-hat at most 1.0020, ess 1807 .. 2168, acceptance 0.68 .. 0.84."""
    m, paths = gp_paths
    res = paths.calibrate(Y, OBS_SD, BOXT, n_chains=FIELD['chains'], n_samples=FIELD['samples'], warmup=FIELD['warmup'], seed=1,
                          method=method, **FKW)
    assert res.x.shape == (6, 4, 1000, 1) and np.all(res.status == 0) and np.all(res.x >= 0.0) and np.all(res.x <= 1.0)
    assert np.array_equal(res.columns, [1]) and np.array_equal(res.controls, CONTROLS) and res.method == method
    W, ybar, w, _, f_grid = whitened_grid(paths)
    z = []
    for p in range(FIELD['J']):
        mean, cov = M.grid_posterior(f_grid[p], [GRID], ybar, w)
        x = res.x[p, :, :, 0]
        z.append((H.zscore(x, mean[0]), H.zscore((x - mean[0]) ** 2, cov[0, 0])))
    z = np.array(z)
    print('%s: acceptance %.2f .. %.2f, ess %.0f .. %.0f, rhat max %.4f (bound %.4f)' %
          (method, res.accept_rate.min(), res.accept_rate.max(), res.ess.min(), res.ess.max(), res.rhat.max(), RHAT_MAX[method]))
    print('z of the means %s, of the variances %s' % (np.round(z[:, 0], 2), np.round(z[:, 1], 2)))
    assert np.max(np.abs(z)) <= MARGIN
    assert np.all(res.rhat < RHAT_MAX[method]) and np.all(res.ess > 100)


def test_field_gp_evidence(eng, gp_paths):
    """calibrate_smc on the same case: per draw log_evidence within 5 CPU['field_logz'] of grid_evidence of the whitened grid
    values; log_norm is the constant of the multivariate normal.  Observed on an MI355X (seed 1): log_evidence - quadrature
    0.017, 0.056, -0.025, 0.013, 0.033, 0.015 against the bound 0.1575."""
    m, paths = gp_paths
    res = paths.calibrate_smc(Y, OBS_SD, BOXT, n_particles=FIELD['particles'], n_moves=FIELD['moves'], seed=1, **FKW)
    assert res.x.shape == (6, 512, 1) and np.all(res.status == 0) and np.all(res.betas[:, -1] == 1.0)
    assert np.array_equal(res.columns, [1]) and np.array_equal(res.controls, CONTROLS)
    W, ybar, w, log_norm, f_grid = whitened_grid(paths)
    assert res.log_norm == pytest.approx(-2.5 * np.log(2.0 * np.pi) - 0.5 * np.linalg.slogdet(SIGMA)[1], rel=1e-13) and \
        res.log_norm == pytest.approx(log_norm, rel=1e-13)
    for p in range(FIELD['J']):
        exact = SMC.grid_evidence(f_grid[p], [GRID], ybar, w)
        print('draw %d: log evidence %.4f, quadrature %.4f (bound %.4f)' % (p, res.log_evidence[p], exact, MARGIN * CPU['field_logz']))
        assert abs(res.log_evidence[p] - exact) <= MARGIN * CPU['field_logz']


# ------------------------------------------------------------------------------------------------ bits
KW = dict(n_chains=4, n_samples=60, warmup=60, n_candidates=128)
NAMES = ('x0', 'x', 'logp', 'accept_rate', 'step', 'status')
SMC_NAMES = ('x', 'loglik', 'logp', 'log_evidence', 'betas', 'stage_ess', 'accept_rate', 'step', 'status')


def same(a, c, names=NAMES):
    return all(np.array_equal(getattr(a, n), getattr(c, n), equal_nan=True) for n in names)


def test_logp_is_the_field_log_posterior(eng, gp_paths):
    """logp of the chains' last samples against -1/2 r^T Sigma^-1 r - the prior's part, r = y - paths(rows), by
    np.linalg.solve.  The slack: the lane form and the matrix form of a draw differ by form_bound per site (the bound of
    tests/test_gpu_calibrate_model.py), which moves the quadratic form by |Sigma^-1 r| . bound + 1/2 bound |Sigma^-1| bound,
    and the whitening's own rounding, 64 T cond eps |logp| (tests/test_boxsites_host.py).  Observed: the largest difference is
    0.00135 of its bound."""
    m, paths = gp_paths
    prior = (np.array([0.5]), np.array([0.2]))
    res = paths.calibrate(Y, OBS_SD, BOXT, seed=3, prior=prior, **KW, **FKW)
    P, R = 6, 4
    theta = res.x[:, :, -1, 0].reshape(-1)
    rows = site_rows(theta)
    own = np.repeat(np.repeat(np.arange(P), R), 5)
    f = B.values_of(paths, rows)[np.arange(len(rows)), own].reshape(P * R, 5)
    bound = B.form_bound(paths, rows)[np.arange(len(rows)), own].reshape(P * R, 5)
    lp = S.field_logp(Y, f[:, :, None], OBS_SD, OBS_COV, theta[:, None], 1.0 / prior[1] ** 2, prior[0])
    Si = np.linalg.inv(SIGMA)
    r = Y[:, 0] - f
    slack = np.sum(np.abs(r @ Si) * bound, 1) + 0.5 * np.einsum('qs,st,qt->q', bound, np.abs(Si), bound) + 64 * 5 * 12.5 * EPS * np.abs(lp)
    diff = np.abs(res.logp[:, :, -1].reshape(-1) - lp)
    print('logp against the field log posterior: largest difference / bound %.3g' % np.max(diff / slack))
    assert np.all(diff <= slack)


def test_replays_and_blocks_change_no_bit(eng, gp_paths, monkeypatch):
    from dgp_amd import calibrate, fieldcal, pathfun
    m, paths = gp_paths
    run = lambda **kw: paths.calibrate(Y, OBS_SD, BOXT, seed=5, **dict(KW, **kw), **FKW)
    whole = run()
    assert same(run(), whole) and not np.array_equal(paths.calibrate(Y, OBS_SD, BOXT, seed=6, **KW, **FKW).x, whole.x)
    for size in (1, 7, 64):                                                      # the rounds of one upload
        monkeypatch.setattr(calibrate, '_rounds_per_upload', lambda Q, Dx, size=size: size)
        assert same(run(), whole), size
    monkeypatch.undo()
    for rows in (5, 13):                                                         # per-path rows per walk call: 1 and 2 chains of the 4
        monkeypatch.setattr(fieldcal, 'MAX_ROWS', rows)
        assert same(run(), whole), rows
    monkeypatch.undo()
    hmc = run(method='hmc', n_leapfrog=3)
    monkeypatch.setattr(fieldcal, 'MAX_ROWS', 5)
    assert same(run(method='hmc', n_leapfrog=3), hmc)
    monkeypatch.undo()
    for rows in (7, 64):                                                         # the shared rows of the candidate screen
        monkeypatch.setattr(pathfun, '_rows_per_call', lambda e, P, width, rows=rows: rows)
        assert same(run(), whole), rows
    monkeypatch.undo()
    dev = run(rng='device')
    assert dev.rng == 'device' and same(run(rng='device'), dev) and not np.array_equal(dev.x, whole.x)
    smc = lambda **kw: paths.calibrate_smc(Y, OBS_SD, BOXT, n_particles=130, n_moves=2, seed=9, **kw, **FKW)
    first = smc()
    assert same(smc(), first, SMC_NAMES)
    monkeypatch.setattr(fieldcal, 'MAX_ROWS', 5 * 33)
    assert same(smc(), first, SMC_NAMES)
    monkeypatch.undo()
    sdev = smc(rng='device')
    assert same(smc(rng='device'), sdev, SMC_NAMES) and not np.array_equal(sdev.x, first.x)


def test_a_draw_does_not_depend_on_the_draws_beside_it(eng, gp_paths):
    """The drivers on the gp's closures with the paths sliced to draws 0 .. 1: their bits are the whole run's.  The chains run
    with rng='device', whose numbers are chain (p, r)'s own; calibrate.Streams draws a slot's numbers for all P paths at once, so
    under rng='numpy' a draw's numbers depend on P (as they do without controls)."""
    import torch
    from dgp_amd import calibrate, fieldcal
    m, paths = gp_paths
    whole = paths.calibrate(Y, OBS_SD, BOXT, seed=7, rng='device', **KW, **FKW)
    e, P, K, Dx, values, vj, width = paths._lane_problem(np.zeros((2, 2)), 'calibrate')
    n = 2

    def first_two(xt):
        f, J = vj(torch.cat([xt, xt.new_zeros(P - n, *xt.shape[1:]) + 0.5], 0))
        return f[:n].contiguous(), J[:n].contiguous()
    W, ybar, w, log_norm = fieldcal.whiten(Y, OBS_SD, OBS_COV, K)
    cc, th = np.array([0]), np.array([1])
    closures = fieldcal.site_closures(e, n, K, Dx, lambda xd: values(xd)[:n], first_two, width, W, CONTROLS, cc, th)
    problem = fieldcal.FieldProblem(5 * K, 1, ybar, w, log_norm, *closures, 5 * width, th, CONTROLS)
    part = calibrate.calibrate(e, n, K, Dx, None, None, None, Y, OBS_SD, BOXT, seed=7, rng='device', problem=problem, **KW)
    for name in NAMES:
        assert np.array_equal(getattr(whole, name)[:n], getattr(part, name)), name
    kw = dict(n_particles=130, n_moves=2, seed=9)
    sp = calibrate.calibrate_smc(e, n, K, Dx, None, None, None, Y, OBS_SD, BOXT, problem=problem, **kw)
    assert np.all(sp.status == 0)
    sw = paths.calibrate_smc(Y, OBS_SD, BOXT, max_stages=sp.n_stages, **kw, **FKW)   # (stopped where the part stops, as the SMC test does)
    for name in SMC_NAMES:
        assert np.array_equal(getattr(sw, name)[:n], getattr(sp, name), equal_nan=True), name


def test_one_site_is_calibrate_with_the_column_pinned(eng, gp_paths):
    """T = 1, obs_cov None, one control column: statistically the posterior of calibrate with that column's bounds pinned
    (lo = hi) at the control value.  The pooled mean and variance of theta of the two runs within 5 standard errors of their
    difference, the errors from every draw's own ess.  Observed: pooled means 0.59212 and 0.59654, z -0.52; pooled variances
    0.03869 and 0.04041, z -0.96."""
    from dgp_amd import calibrate
    m, paths = gp_paths
    kw = dict(n_chains=4, n_samples=400, warmup=300, n_candidates=128)
    c, y, sd = 0.45, 0.06, 0.05
    field = paths.calibrate([[y]], sd, BOXT, seed=11, controls=[[c]], control_columns=[0], **kw)
    pinned = paths.calibrate(y, sd, np.array([[c, c], [0.0, 1.0]]), seed=12, **kw)
    assert np.all(field.status == 0) and np.all(pinned.status == 0) and np.all(pinned.x[..., 0] == c)
    a, b = field.x[..., 0], pinned.x[..., 1]                                     # (P, R, S) each
    centre = 0.5 * (a.mean() + b.mean())

    def pooled(series):
        """(the mean over the draws of their own means, its standard error)."""
        se2 = [s.var() / calibrate.ess(s) for s in series]
        return np.mean([s.mean() for s in series]), np.sqrt(np.sum(se2)) / len(series)
    for what, fa, fb in (('mean', a, b), ('variance', (a - centre) ** 2, (b - centre) ** 2)):
        (ma, sa), (mb, sb) = pooled(fa), pooled(fb)
        z = (ma - mb) / np.hypot(sa, sb)
        print('one site against the pinned column, pooled %s: %.5f and %.5f, z %.2f' % (what, ma, mb, z))
        assert abs(z) <= MARGIN


# ------------------------------------------------------------------------------------------------ emulators
SHORT = dict(n_chains=4, n_samples=40, warmup=40, n_candidates=128)


@pytest.fixture(scope='module', params=['two-connect', 'three'])
def emu_paths(request, eng):
    from dgp_amd import emulator
    X, model = T._model(request.param)
    emu = emulator(model.estimate(), N=2, seed=5)
    return request.param, emu, emu.sample_functions(sample_size=3, n_features=100)


def test_emulator_field_calibration(eng, emu_paths):
    which, emu, paths = emu_paths
    controls = np.array([[0.2], [0.5], [0.8], [0.5]])                            # (the last repeats the second: a replicate)
    vals = B.values_of(paths, np.column_stack([controls[:, 0], np.full(4, 0.4)]))
    y = np.median(vals, 1)[:, None] + np.array([[0.01], [-0.02], [0.0], [0.015]])
    cov = 0.03 ** 2 * np.exp(-(controls - controls.T) ** 2 / (2.0 * 0.3 ** 2))
    fkw = dict(controls=controls, control_columns=[0], obs_cov=cov)
    res = paths.calibrate(y, 0.05, BOXT, seed=7, **SHORT, **fkw)
    assert res.x.shape == (6, 4, 40, 1) and res.logp.shape == (6, 4, 40) and res.x0.shape == (6, 4, 1)
    assert np.all(res.x >= 0.0) and np.all(res.x <= 1.0) and np.all(res.status == 0) and np.all(np.isfinite(res.logp))
    assert np.array_equal(res.columns, [1]) and np.array_equal(res.controls, controls) and res.rounds == 81
    assert same(paths.calibrate(y, 0.05, BOXT, seed=7, **SHORT, **fkw), res)
    # a NaN entry of y is ignored: the run is the run without that site, bit for bit (its rows are evaluated and not read)
    gap = np.array([[0.35]])
    y5, c5 = np.concatenate([y[:2], [[np.nan]], y[2:]]), np.concatenate([controls[:2], gap, controls[2:]])
    cov5 = 0.03 ** 2 * np.exp(-(c5 - c5.T) ** 2 / (2.0 * 0.3 ** 2))
    assert same(paths.calibrate(y5, 0.05, BOXT, seed=7, controls=c5, control_columns=[0], obs_cov=cov5, **SHORT), res)
    smc = paths.calibrate_smc(y, 0.05, BOXT, n_particles=64, n_moves=2, seed=3, **fkw)
    assert smc.x.shape == (6, 64, 1) and np.all(smc.status == 0) and np.all(smc.x >= 0.0) and np.all(smc.x <= 1.0)
    assert np.all(np.isfinite(smc.log_evidence)) and np.isfinite(smc.log_norm) and np.array_equal(smc.columns, [1])
    e5 = paths.calibrate_smc(y5, 0.05, BOXT, n_particles=64, n_moves=2, seed=3, controls=c5, control_columns=[0], obs_cov=cov5)
    assert same(e5, smc, SMC_NAMES) and e5.log_norm == pytest.approx(smc.log_norm, rel=1e-12)
    hm = emu.calibrate(y, 0.05, BOXT, sample_size=2, n_features=64, seed=1, method='hmc', n_leapfrog=3, **SHORT, **fkw)
    assert hm.x.shape == (4, 4, 40, 1) and np.all(hm.status == 0) and np.array_equal(hm.columns, [1])
    # the refusals
    for bad in (dict(obs_cov=cov, controls=None, control_columns=None), dict(control_columns=None), dict(control_columns=[0, 1]),
                dict(control_columns=[2]), dict(controls=controls[:, 0]), dict(controls=np.full((4, 1), np.nan)),
                dict(obs_cov=-np.eye(4)), dict(obs_cov=np.eye(3)), dict(obs_cov=np.triu(np.ones((4, 4))))):
        with pytest.raises(ValueError):
            paths.calibrate(y, 0.05, BOXT, **SHORT, **dict(fkw, **bad))
    for yy, sd, box in ((y[:3], 0.05, BOXT), (y, np.ones(3), BOXT), (y, 0.0, BOXT), (np.full((4, 1), np.nan), 0.05, BOXT),
                        (y, 0.05, np.array([[1.0, 0.0]]))):
        with pytest.raises(ValueError):
            paths.calibrate(yy, sd, box, **SHORT, **fkw)
    with pytest.raises(ValueError):
        paths.calibrate_smc(y, 0.05, BOXT, n_particles=64, obs_cov=cov)
    with pytest.raises(ValueError):
        paths.calibrate(y, 0.05, BOXT, x0=np.zeros((4, 2)), **SHORT, **fkw)      # x0 has Dtheta columns


def test_the_refusals_of_calibrate_are_unchanged(eng, gp_paths):
    from dgp_amd import emulator
    m, paths = gp_paths
    np.random.seed(1)
    local = m.sample_functions_vecchia(sample_size=2, n_features=16, m=10)
    with pytest.raises(NotImplementedError, match='sample_functions '):
        local.calibrate(Y, OBS_SD, BOXT, **SHORT, **FKW)
    with pytest.raises(NotImplementedError, match='sample_functions '):
        local.calibrate_smc(Y, OBS_SD, BOXT, n_particles=64, **FKW)
    X, model = T._model('hetero')
    emu = emulator(model.estimate(), N=2, seed=5)
    with pytest.raises(ValueError, match='sampled node'):
        emu.sample_functions(sample_size=2, n_features=16).calibrate(Y, OBS_SD, BOXT, **SHORT, **FKW)
    res = m.calibrate(Y[:, 0], OBS_SD, BOXT, sample_size=3, n_features=64, seed=2, **SHORT, **FKW)       # gp.calibrate: y (T,)
    assert res.x.shape == (3, 4, 40, 1) and np.array_equal(res.columns, [1])
