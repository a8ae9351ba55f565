"""paths.calibrate_smc, emulator.calibrate_smc and gp.calibrate_smc (dgp_amd/calibrate.py, DESIGN I.21) on the small models
of tests/test_gpu_calibrate_model.py: every draw's evidence, mode masses and moments against quadrature on a grid of the
draw's own values, the log densities against paths(x), the tempering schedule, replays and invariances, the prior, the
sufficient statistics and the refusals.  Needs an MI355X: -m gpu.

The statistical bounds are 5 x the spread over seeds that the numpy restatement (tests/boxsmc_ref.py) shows on the same
draws, replayed in numpy, with the same settings: CPU below, measured by tests/test_boxsmc_host.py
(test_line_gp_on_the_cpu, test_bimodal_gp_on_the_cpu), which also holds these numbers to what it measures."""
import types

import numpy as np
import pytest

import boxmala_ref as M
import boxsmc_ref as S
import pathfun_ref as Rf
import pathgrad_ref as Rg
import test_gpu_boxmin_model as B
import test_gpu_calibrate_model as C
import test_gpu_pathfun as T

pytestmark = pytest.mark.gpu
MARGIN = 5.0
LINE, GRID, BOX1, BOX = C.LINE, C.GRID, C.BOX1, C.BOX
SMC = dict(n_particles=512, n_moves=4)
BIMODAL = dict(J=6, F=128, seed=29, y=0.49, sd=0.02)
# Over 16 seeds of the restatement, the largest over the 6 draws of: the standard deviation of log_evidence; of the particles'
# mean and variance, in units of sqrt(var / R) and var sqrt(2 / R) (the inflation over R independent samples); of the mass
# of x < 0.5.
CPU = dict(line_logz=0.0869, line_mean=1.32, line_var=1.40, bimodal_logz=0.141, bimodal_mass=0.0737)
SMALL = dict(n_particles=64, n_moves=2)


@pytest.fixture(scope='module')
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    from dgp_amd.ops import default_engine
    return default_engine(0)


def bimodal(n=30):
    X = np.linspace(0.0, 1.0, n)[:, None]
    return X, (2.0 * X - 1.0) ** 2


def gp_case(X, Y, seed, J, F):
    """The fixed-hyperparameter gp of T._gp on (X, Y) and its draws under np.random.seed(seed), in numpy:
    (funs[p](x (R, 1)) -> (values (R, 1), Jacobian (R, 1, 1)) of draw p, the draws on GRID (J, 4001))."""
    kind, length, scale, nugget = 'sexp', np.full(1, 0.7), 1.9, 1e-4
    k = types.SimpleNamespace(name=kind, length=length, _X=lambda: X)
    _, Omega, b, theta, eps = T._gp_replay(types.SimpleNamespace(kernel=k), seed, J, F)
    v = Rf.weights(X, Y[:, 0], Omega, b, theta, eps, kind, length, scale, nugget, None)
    funs = [lambda x, p=p: (Rf.evaluate(x, X, Omega, b, theta[p:p + 1], v[p:p + 1], kind, length, scale)[0][:, None],
                            Rg.grad(x, X, Omega, b, theta[p:p + 1], v[p:p + 1], kind, length, scale)[0][:, None, :])
            for p in range(J)]
    return funs, Rf.evaluate(GRID[:, None], X, Omega, b, theta, v, kind, length, scale)


def obs(case):
    return np.array([case['y']]), np.array([1.0 / case['sd'] ** 2])


# ------------------------------------------------------------------------------------------------ the 1-D gps
def test_line_gp_against_quadrature(eng):
    """6 draws, 512 particles: per draw log_evidence within 5 CPU['line_logz'] of grid_evidence over paths(GRID), and the
    particles' mean and variance within 5 standard errors of grid_posterior's, the standard error that of 512 independent
    samples times the inflation the restatement shows."""
    X, Y = C.line()
    m = T._gp('sexp', X, Y)
    np.random.seed(LINE['seed'])
    paths = m.sample_functions(sample_size=LINE['J'], n_features=LINE['F'])
    res = paths.calibrate_smc(LINE['y'], LINE['sd'], BOX1, seed=1, **SMC)
    R = SMC['n_particles']
    assert res.x.shape == (6, R, 1) and np.all(res.status == 0) and np.all(res.betas[:, -1] == 1.0)
    f_grid = paths(GRID[:, None])
    ybar, w = obs(LINE)
    for p in range(LINE['J']):
        exact = S.grid_evidence(f_grid[:, p], [GRID], ybar, w)
        mean, cov = M.grid_posterior(f_grid[:, p], [GRID], ybar, w)
        x = res.x[p, :, 0]
        zm = (x.mean() - mean[0]) / (np.sqrt(cov[0, 0] / R) * CPU['line_mean'])
        zv = (x.var() - cov[0, 0]) / (cov[0, 0] * np.sqrt(2.0 / R) * CPU['line_var'])
        print('draw %d: log evidence %.4f, quadrature %.4f (bound %.4f); z of the mean %.2f, of the variance %.2f; stages %d'
              % (p, res.log_evidence[p], exact, MARGIN * CPU['line_logz'], zm, zv, np.sum(np.isfinite(res.stage_ess[p]))))
        assert abs(res.log_evidence[p] - exact) <= MARGIN * CPU['line_logz']
        assert abs(zm) <= MARGIN and abs(zv) <= MARGIN


def test_bimodal_gp_keeps_both_modes(eng):
    """A gp trained on (2x - 1)^2, y = 0.49, obs_sd = 0.02: the posterior of every draw has a mode near 0.15 and one near
    0.85.  Per draw the mass of x < 0.5 and log_evidence within 5 x the restatement's spread of quadrature over the draw's
    own grid values; every draw keeps particles in both modes.  For the record (printed, not asserted): MALA chains started
    in the left mode stay there."""
    X, Y = bimodal()
    m = T._gp('sexp', X, Y)
    np.random.seed(BIMODAL['seed'])
    paths = m.sample_functions(sample_size=BIMODAL['J'], n_features=BIMODAL['F'])
    res = paths.calibrate_smc(BIMODAL['y'], BIMODAL['sd'], BOX1, seed=2, **SMC)
    assert np.all(res.status == 0)
    f_grid = paths(GRID[:, None])
    ybar, w = obs(BIMODAL)
    for p in range(BIMODAL['J']):
        exact, mass = S.grid_evidence(f_grid[:, p], [GRID], ybar, w), S.grid_mass(f_grid[:, p], [GRID], ybar, w, 0.5)
        left = np.mean(res.x[p, :, 0] < 0.5)
        print('draw %d: mass of x < 0.5 %.3f, quadrature %.3f (bound %.3f); log evidence %.4f, quadrature %.4f (bound %.4f)'
              % (p, left, mass, MARGIN * CPU['bimodal_mass'], res.log_evidence[p], exact, MARGIN * CPU['bimodal_logz']))
        assert abs(left - mass) <= MARGIN * CPU['bimodal_mass']
        assert abs(res.log_evidence[p] - exact) <= MARGIN * CPU['bimodal_logz']
        assert 0 < np.sum(res.x[p, :, 0] < 0.5) < SMC['n_particles']
    x0 = np.full((4, 1), 0.15)
    chains = paths.calibrate(BIMODAL['y'], BIMODAL['sd'], BOX1, x0=x0, n_samples=200, warmup=200, seed=2)
    print('calibrate(method=mala) from x0 = 0.15: mass of x < 0.5 per draw %s' % np.round(np.mean(chains.x[..., 0] < 0.5, (1, 2)), 3))
    sharp = paths.calibrate_smc(BIMODAL['y'], BIMODAL['sd'], BOX1, seed=2, max_stages=1, **SMC)
    assert np.all(sharp.status == 2) and np.all(sharp.betas[:, -1] < 1.0) and sharp.n_stages == 1
    assert np.all(sharp.draw_weights() == 0.0)


# ------------------------------------------------------------------------------------------------ 2-D models
@pytest.fixture(scope='module')
def gp_paths(eng):
    X, Y = B.bowl()
    m = T._gp('sexp', X, Y)
    np.random.seed(31)
    return m, m.sample_functions(sample_size=6, n_features=128)


@pytest.fixture(scope='module', params=['two-connect', 'three'])
def emu_paths(request, eng):
    from dgp_amd import emulator
    X, model = T._model(request.param)
    emu = emulator(model.estimate(), N=2, seed=5)
    return request.param, emu, emu.sample_functions(sample_size=3, n_features=100)


NAMES = ('x', 'loglik', 'logp', 'log_evidence', 'betas', 'stage_ess', 'accept_rate', 'step', 'status')


def same(a, c, rows=slice(None)):
    return all(np.array_equal(getattr(a, n)[rows], getattr(c, n), equal_nan=True) for n in NAMES) and a.n_stages == c.n_stages


def check_particles(obj, res, y, sd, P, kw, prior=None, ess_frac=0.5):
    """What every result must satisfy, against the draws' own shared-rows evaluation."""
    R = kw['n_particles']
    lo, hi = BOX[:, 0], BOX[:, 1]
    Tn = res.n_stages
    assert res.x.shape == (P, R, 2) and res.loglik.shape == (P, R) and res.logp.shape == (P, R) and res.step.shape == (P, R)
    assert all(getattr(res, n).shape == (P, Tn) for n in ('betas', 'stage_ess', 'accept_rate'))
    assert res.log_evidence.shape == (P,) and res.status.shape == (P,) and res.pooled().shape == (P * R, 2)
    assert res.evaluations == Tn * (kw['n_moves'] + 1)
    assert np.all(res.x >= lo) and np.all(res.x <= hi) and np.all(res.status == 0) and np.all(res.step > 0.0)
    assert np.all(np.isfinite(res.log_evidence)) and np.all(res.log_evidence <= 0.0)         # (ll <= 0 under a normalised prior)
    # beta increases to exactly 1; a stage keeps ESS >= ess_frac R up to the rounding of the device's sums (test_gpu_boxsmc.py)
    assert np.all(np.diff(res.betas, axis=1) >= 0.0) and np.all(res.betas[:, -1] == 1.0) and np.all(res.betas[:, 0] > 0.0)
    stepped = np.isfinite(res.stage_ess)
    assert stepped[:, 0].all() and np.all(res.stage_ess[stepped] >= ess_frac * R * (1.0 - (4 * R + 6000) * 2.0 ** -52))
    assert np.all(res.stage_ess[stepped] <= R * (1.0 + (4 * R + 6000) * 2.0 ** -52))
    assert np.all(stepped[:, 1:] <= (res.betas[:, :-1] < 1.0))                               # NaN once a draw has finished
    assert abs(res.draw_weights().sum() - 1.0) <= 1e-14 and 1.0 <= res.draw_ess <= P * (1.0 + 1e-14)
    assert res.pooled_weights().shape == (P * R,) and abs(res.pooled_weights().sum() - 1.0) <= 1e-12
    # loglik and logp: the draw's own values, as paths(x) gives them at the final particles (row p R + r belongs to path p)
    rows = res.x.reshape(P * R, 2)
    own = np.repeat(np.arange(P), R)
    f = B.values_of(obj, rows)[np.arange(P * R), own]
    bound = B.form_bound(obj, rows)[np.arange(P * R), own]
    w = 1.0 / sd ** 2
    ll = -0.5 * w * (y - f) ** 2
    lp = ll if prior is None else ll - 0.5 * np.sum((rows - prior[0]) ** 2 / prior[1] ** 2, 1)
    slack = w * np.abs(y - f) * bound + 0.5 * w * bound ** 2 + 16 * np.finfo(float).eps * np.abs(lp)
    d1, d2 = np.abs(res.loglik.reshape(-1) - ll), np.abs(res.logp.reshape(-1) - lp)
    print('loglik, logp against paths(x): largest difference / bound %.3g, %.3g' % (np.max(d1 / slack), np.max(d2 / slack)))
    assert np.all(d1 <= slack) and np.all(d2 <= slack)


def evidence_bound(res):
    """(P,): 5 standard deviations of log_evidence by the delta method on the stages' own weights: a stage's mean weight over R
    independent particles has relative variance (R / ESS_t - 1) / R, and the stages add.  It ignores what resampling and
    unmixed moves add; the restatement's spread over 16 seeds is 1.3 times it on draw 0 of the line gp and of the bimodal gp
    (0.083 against 0.063, 0.101 against 0.078) and at most 1.8 times on their worst draws, well inside the factor 5."""
    R = res.x.shape[1]
    return MARGIN * np.sqrt(np.nansum((R / res.stage_ess - 1.0) / R, 1))


def test_gp_calibrate_smc(eng, gp_paths):
    m, paths = gp_paths
    kw = dict(n_particles=256, n_moves=3)
    res = paths.calibrate_smc(0.05, 0.05, BOX, seed=3, **kw)
    check_particles(paths, res, 0.05, 0.05, 6, kw)
    assert same(res, paths.calibrate_smc(0.05, 0.05, BOX, seed=3, **kw))             # the same arguments: the same bits
    assert not np.array_equal(res.x, paths.calibrate_smc(0.05, 0.05, BOX, seed=4, **kw).x)
    r2 = np.sum((res.pooled() - np.array([0.3, 0.6])) ** 2, 1)                   # the ring of the bowl, as calibrate finds it
    assert abs(np.median(r2) - 0.05) < 0.03
    # the evidence against quadrature on a 2-D grid of the draws' own values
    g = np.linspace(0.0, 1.0, 201)
    mesh = np.stack(np.meshgrid(g, g, indexing='ij'), -1).reshape(-1, 2)
    f_grid = paths(mesh)
    ybar, w = np.array([0.05]), np.array([400.0])
    exact = np.array([S.grid_evidence(f_grid[:, p], [g, g], ybar, w) for p in range(6)])
    print('log evidence %s, quadrature %s, bounds %s' % (np.round(res.log_evidence, 3), np.round(exact, 3), np.round(evidence_bound(res), 3)))
    assert np.all(np.abs(res.log_evidence - exact) <= evidence_bound(res))
    s = res.summary(0.9, weights='evidence')
    assert all(s[k].shape == (2,) for k in ('mean', 'lower', 'upper', 'draw_sd')) and np.all(s['lower'] < s['mean']) and np.all(s['mean'] < s['upper'])
    assert res.resample(50, seed=1).shape == (50, 2)


def test_a_draw_does_not_depend_on_the_draws_beside_it(eng, gp_paths):
    """The driver on the gp's closures with the paths sliced to draws 2 .. 3: their bits are the whole run's."""
    from dgp_amd import calibrate
    m, paths = gp_paths
    kw = dict(n_particles=130, n_moves=2, seed=9)
    whole = paths.calibrate_smc(0.05, 0.05, BOX, **kw)
    e, P, K, Dx, values, vj, width = paths._lane_problem(BOX, 'calibrate_smc')
    a, c = 0, 2                                                                  # (the streams give draw p the numbers of row p)

    def first_two(xt):
        import torch
        full = torch.cat([xt, xt.new_zeros(P - (c - a), *xt.shape[1:]) + 0.5], 0)
        f, J = vj(full)
        return f[a:c].contiguous(), J[a:c].contiguous()
    part = calibrate.calibrate_smc(e, c - a, K, Dx, values, first_two, width, np.reshape(0.05, (-1, 1)), 0.05, BOX, **kw)
    # (the whole run would go on until its last draw is at beta = 1, moving the others at beta = 1: stop it where the part stops)
    assert np.all(part.status == 0) and part.n_stages <= whole.n_stages
    whole = paths.calibrate_smc(0.05, 0.05, BOX, max_stages=part.n_stages, **kw)
    assert same(whole, part, slice(a, c))


def test_gp_observation_and_prior(eng, gp_paths):
    from dgp_amd import calibrate
    m, paths = gp_paths
    kw = dict(n_particles=256, n_moves=3)
    y = 0.05 + 0.02 * np.random.default_rng(8).normal(size=(4, 1))               # T = 4 replicates at the same unknown x
    ybar = calibrate.observation(y, 0.1, 1)[0]
    rep, mean = paths.calibrate_smc(y, 0.1, BOX, seed=2, **kw), paths.calibrate_smc(ybar, 0.05, BOX, seed=2, **kw)
    assert same(rep, mean) and rep.log_norm != mean.log_norm
    assert abs(rep.log_norm - calibrate.log_norm(y, 0.1, 1)) == 0.0
    gaps = paths.calibrate_smc(np.concatenate([y, [[np.nan]]]), 0.1, BOX, seed=2, **kw)  # an unobserved entry is ignored
    assert same(gaps, rep) and gaps.log_norm == rep.log_norm
    # a Gaussian prior shifts the posterior and changes the evidence by the quadrature amount
    prior = (np.array([0.45, 0.5]), np.array([0.1, np.inf]))
    flat, pulled = paths.calibrate_smc(0.05, 0.05, BOX, seed=2, **kw), paths.calibrate_smc(0.05, 0.05, BOX, seed=2, prior=prior, **kw)
    check_particles(paths, pulled, 0.05, 0.05, 6, kw, (prior[0], prior[1]))
    g = np.linspace(0.0, 1.0, 201)
    f_grid = paths(np.stack(np.meshgrid(g, g, indexing='ij'), -1).reshape(-1, 2))
    ybar, w = np.array([0.05]), np.array([400.0])
    pv, pm = np.array([100.0, 0.0]), prior[0]
    change = np.array([S.grid_evidence(f_grid[:, p], [g, g], ybar, w, pv, pm) - S.grid_evidence(f_grid[:, p], [g, g], ybar, w) for p in range(6)])
    got = pulled.log_evidence - flat.log_evidence
    bound = np.sqrt(evidence_bound(pulled) ** 2 + evidence_bound(flat) ** 2)
    print('the prior changes log evidence by %s, quadrature %s, bounds %s' % (np.round(got, 3), np.round(change, 3), np.round(bound, 3)))
    assert np.all(np.abs(got - change) <= bound) and np.all(np.abs(change) > 0.0)
    assert abs(pulled.pooled()[:, 0].mean() - 0.45) < abs(flat.pooled()[:, 0].mean() - 0.45) + 0.02


def test_emulator_calibrate_smc(eng, emu_paths):
    import copy
    which, emu, paths = emu_paths
    y = float(np.median(B.values_of(paths, np.random.default_rng(1).uniform(size=(64, 2)))))    # a value the draws do take
    kw = dict(n_particles=128, n_moves=2)
    res = paths.calibrate_smc(y, 0.05, BOX, seed=7, **kw)
    check_particles(paths, res, y, 0.05, 6, kw)
    assert same(res, paths.calibrate_smc(y, 0.05, BOX, seed=7, **kw))
    assert not np.array_equal(res.x, paths.calibrate_smc(y, 0.05, BOX, seed=8, **kw).x)
    state = copy.deepcopy(emu._sample_rng)
    fresh = emu.calibrate_smc(y, 0.05, BOX, sample_size=2, n_features=64, seed=1, **SMALL)       # N = 2: four draws
    assert fresh.x.shape == (4, 64, 2) and np.all(fresh.x >= 0.0) and np.all(fresh.x <= 1.0)
    emu._sample_rng = state
    assert same(emu.calibrate_smc(y, 0.05, BOX, sample_size=2, n_features=64, seed=1, **SMALL), fresh)
    with pytest.raises(ValueError):
        paths.calibrate_smc([y, y], 0.05, BOX, **SMALL)                          # one output
    with pytest.raises(ValueError):
        paths.calibrate_smc(y, 0.05, BOX[:1], **SMALL)


def test_refusals(eng, gp_paths):
    from dgp_amd import calibrate, emulator
    m, paths = gp_paths
    np.random.seed(8)
    res = m.calibrate_smc(0.05, 0.05, BOX, sample_size=5, n_features=64, seed=2, **SMALL)
    assert res.x.shape == (5, 64, 2)
    for bad in (BOX[0], BOX[:1], np.array([[0.0, 1.0], [np.nan, 1.0]]), np.array([[0.0, 1.0], [1.0, 0.5]])):
        with pytest.raises(ValueError):
            paths.calibrate_smc(0.05, 0.05, bad, **SMALL)
    for kw in (dict(n_particles=0), dict(n_particles=calibrate.MAX_PARTICLES + 1), dict(n_moves=0), dict(ess_frac=0.0), dict(ess_frac=1.0),
               dict(ess_frac=np.nan), dict(max_stages=0), dict(scale=np.ones(3)), dict(prior=(np.zeros(2), np.zeros(2))),
               dict(prior=(np.zeros(3), np.ones(3))), dict(step=0.0), dict(target_accept=1.0)):
        with pytest.raises(ValueError):
            paths.calibrate_smc(0.05, 0.05, BOX, **dict(SMALL, **kw))
    for y, sd in ((np.nan, 0.05), (np.zeros((2, 2)), 0.05), (0.05, 0.0), (0.05, np.ones(2))):
        with pytest.raises(ValueError):
            paths.calibrate_smc(y, sd, BOX, **SMALL)
    np.random.seed(1)
    local = m.sample_functions_vecchia(sample_size=2, n_features=16, m=10)
    with pytest.raises(NotImplementedError, match='sample_functions '):
        local.calibrate_smc(0.05, 0.05, BOX, **SMALL)
    X, model = T._model('hetero')
    emu = emulator(model.estimate(), N=2, seed=5)
    with pytest.raises(ValueError, match='sampled node'):
        emu.calibrate_smc(0.1, 0.1, np.array([[0.0, 1.0]]), sample_size=2, n_features=16, **SMALL)
