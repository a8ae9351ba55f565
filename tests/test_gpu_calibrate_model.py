"""paths.calibrate, emulator.calibrate and gp.calibrate (dgp_amd/calibrate.py, DESIGN I.19) on small models: every draw's
posterior against quadrature on a grid of the draw's own values, the log densities against paths(x), bit-for-bit replays and
invariances, the sufficient statistics, the prior, and the refusals.  Needs an MI355X: -m gpu.

The device's walk and the numpy restatement's differ in the last bits, so their trajectories part at the first decision that
flips: nothing here compares trajectories with the restatement.  The 1-D comparison is held on the CPU first, with the
restatement driven by pathfun_ref / pathgrad_ref (tests/test_calibrate_host.py::test_line_case_on_the_cpu)."""
import types

import numpy as np
import pytest

import boxmala_ref as M
import pathfun_ref as Rf
import pathgrad_ref as Rg
import test_boxmala_host as H
import test_gpu_boxmin_model as B
import test_gpu_pathfun as T

pytestmark = pytest.mark.gpu
MARGIN = 5.0
RHAT_MAX = 1.01       # (the CPU run's split R-hat lay in 0.9994 .. 1.0010: test_line_case_on_the_cpu; ten times its distance from 1)
LINE = dict(J=6, F=128, seed=23, y=0.1, sd=0.1, chains=4, samples=1000, warmup=500)
GRID = np.linspace(0.0, 1.0, 4001)
BOX1 = np.array([[0.0, 1.0]])
BOX = B.BOX


@pytest.fixture(scope='module')
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    from dgp_amd.ops import default_engine
    return default_engine(0)


# ------------------------------------------------------------------------------------------------ the 1-D gp
def line(n=30):
    X = np.linspace(0.0, 1.0, n)[:, None]
    return X, 2.0 * X - 1.0 + 0.2 * np.sin(3.0 * X)


def line_case():
    """The fixed-hyperparameter gp on the line and its draws under np.random.seed(LINE['seed']), in numpy:
    (funs[p](x (1,)) -> (values (1,), Jacobian (1, 1)) of draw p, the draws on GRID (J, 4001))."""
    X, Y = line()
    kind, length, scale, nugget = 'sexp', np.full(1, 0.7), 1.9, 1e-4
    k = types.SimpleNamespace(name=kind, length=length, _X=lambda: X)
    _, Omega, b, theta, eps = T._gp_replay(types.SimpleNamespace(kernel=k), LINE['seed'], LINE['J'], LINE['F'])
    v = Rf.weights(X, Y[:, 0], Omega, b, theta, eps, kind, length, scale, nugget, None)
    funs = [lambda x, p=p: (Rf.evaluate(x[None], X, Omega, b, theta[p:p + 1], v[p:p + 1], kind, length, scale)[0],
                            Rg.grad(x[None], X, Omega, b, theta[p:p + 1], v[p:p + 1], kind, length, scale)[0])
            for p in range(LINE['J'])]
    return funs, Rf.evaluate(GRID[:, None], X, Omega, b, theta, v, kind, length, scale)


def against_the_grid(x, f_grid):
    """(z of the mean, z of the variance) of the samples x (R, S) of one draw against quadrature of its values on GRID."""
    w, ybar = np.array([1.0 / LINE['sd'] ** 2]), np.array([LINE['y']])
    mean, cov = M.grid_posterior(f_grid, [GRID], ybar, w)
    return H.zscore(x, mean[0]), H.zscore((x - mean[0]) ** 2, cov[0, 0])


def test_line_gp_against_quadrature(eng):
    """6 draws x 4 chains x 1000 samples: per draw the pooled mean and variance (the standard deviation's square) within 5
    standard errors, by the samples' own ess, of their quadrature over paths(GRID); split R-hat below the CPU run's bound.  Observed on an MI355X (seed 1): z of the
    means -0.32, 0.02, -0.10, -1.26, 2.33, 0.69, of the variances -1.68, 0.64, 0.05, 0.28, -0.80, -0.23; split R-hat at most
    1.0010; ess 2326 .. 2919 of 4000; acceptance 0.47 .. 0.70."""
    X, Y = line()
    m = T._gp('sexp', X, Y)
    np.random.seed(LINE['seed'])
    paths = m.sample_functions(sample_size=LINE['J'], n_features=LINE['F'])
    res = paths.calibrate(LINE['y'], LINE['sd'], BOX1, n_chains=LINE['chains'], n_samples=LINE['samples'], warmup=LINE['warmup'], seed=1)
    assert res.x.shape == (6, 4, 1000, 1) and np.all(res.status == 0) and res.rounds == 1501
    f_grid = paths(GRID[:, None])
    z = np.array([against_the_grid(res.x[p, :, :, 0], f_grid[:, p]) for p in range(LINE['J'])])
    print('line gp: acceptance %.2f .. %.2f, steps %.3g .. %.3g, ess %.0f .. %.0f, rhat max %.4f' %
          (res.accept_rate.min(), res.accept_rate.max(), res.step.min(), res.step.max(), res.ess.min(), res.ess.max(), res.rhat.max()))
    print('z of the means %s, of the variances %s' % (np.round(z[:, 0], 2), np.round(z[:, 1], 2)))
    assert np.max(np.abs(z)) <= MARGIN
    assert np.all(res.rhat < RHAT_MAX) and np.all(res.ess > 100)
    assert np.all(res.accept_rate > 0.3) and np.all(res.accept_rate < 0.85)


# ------------------------------------------------------------------------------------------------ 2-D models
KW = dict(n_chains=4, n_samples=100, warmup=100, n_candidates=256)
SHORT = dict(n_chains=4, n_samples=40, warmup=40, n_candidates=256)


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


def same(a, c):
    return all(np.array_equal(getattr(a, n), getattr(c, n)) for n in ('x0', 'x', 'logp', 'accept_rate', 'step', 'status'))


def check_posterior(obj, res, y, sd, P, kw, prior=None):
    """What every result must satisfy, against the draws' own shared-rows evaluation."""
    R, S = kw['n_chains'], kw['n_samples']
    lo, hi = BOX[:, 0], BOX[:, 1]
    assert res.x.shape == (P, R, S, 2) and res.logp.shape == (P, R, S) and res.x0.shape == (P, R, 2)
    assert all(getattr(res, n).shape == (P, R) for n in ('accept_rate', 'step', 'status')) and res.rounds == 1 + kw['warmup'] + S
    assert res.rhat.shape == (P, 2) and res.ess.shape == (P, 2) and res.pooled().shape == (P * R * S, 2)
    assert np.all(res.x >= lo) and np.all(res.x <= hi) and np.all(res.status == 0)
    assert np.all(res.accept_rate > 0.0) and np.all(res.accept_rate < 1.0) and np.all(res.step > 0.0)
    # logp: the draw's own values, as paths(x) gives them at the chains' last samples (row p R + r belongs to path p)
    rows = res.x[:, :, -1].reshape(P * R, 2)
    own = np.repeat(np.arange(P), R)
    f = B.values_of(obj, rows)[np.arange(P * R), own]
    bound = B.form_bound(obj, rows)[np.arange(P * R), own]
    w = 1.0 / sd ** 2
    lp = -0.5 * w * (y - f) ** 2
    if prior is not None:
        lp = lp - 0.5 * np.sum((rows - prior[0]) ** 2 / prior[1] ** 2, 1)
    slack = w * np.abs(y - f) * bound + 0.5 * w * bound ** 2 + 16 * np.finfo(float).eps * np.abs(lp)
    diff = np.abs(res.logp[:, :, -1].reshape(-1) - lp)
    print('logp against paths(x): largest difference / bound %.3g' % np.max(diff / slack))
    assert np.all(diff <= slack)


def test_gp_calibrate(eng, gp_paths):
    m, paths = gp_paths
    res = paths.calibrate(0.05, 0.05, BOX, seed=3, **KW)
    check_posterior(paths, res, 0.05, 0.05, 6, KW)
    assert same(res, paths.calibrate(0.05, 0.05, BOX, seed=3, **KW))             # the same arguments: the same bits
    assert not np.array_equal(res.x, paths.calibrate(0.05, 0.05, BOX, seed=4, **KW).x)
    # the samples lie around the ring (x0 - 0.3)^2 + (x1 - 0.6)^2 = 0.05 of the bowl
    r2 = np.sum((res.pooled() - np.array([0.3, 0.6])) ** 2, 1)
    assert abs(np.median(r2) - 0.05) < 0.03
    q = paths.calibrate(0.05, 0.05, BOX, seed=3, qmc=True, **KW)
    assert q.x.shape == res.x.shape and np.all(q.x >= 0.0) and np.all(q.x <= 1.0)
    thinned = paths.calibrate(0.05, 0.05, BOX, seed=3, thin=3, **dict(KW, n_samples=20))
    assert thinned.x.shape == (6, 4, 20, 2) and thinned.rounds == 1 + 100 + 60
    assert np.array_equal(thinned.x[:, :, :20], res.x[:, :, 2:60:3])             # every third round of the same chains


def test_gp_blocks_and_starts_change_no_bit(eng, gp_paths, monkeypatch):
    from dgp_amd import calibrate, pathfun
    m, paths = gp_paths
    whole = paths.calibrate(0.05, 0.05, BOX, seed=5, **KW)
    for size in (1, 7, 64):
        monkeypatch.setattr(calibrate, '_rounds_per_upload', lambda Q, Dx, size=size: size)
        assert same(paths.calibrate(0.05, 0.05, BOX, seed=5, **KW), whole), size
    monkeypatch.undo()
    for rows in (7, 64, 200):
        monkeypatch.setattr(pathfun, '_rows_per_call', lambda e, P, width, rows=rows: rows)
        assert same(paths.calibrate(0.05, 0.05, BOX, seed=5, **KW), whole), rows
    monkeypatch.undo()
    x0 = np.random.default_rng(4).uniform(size=(4, 2))
    four, two = paths.calibrate(0.05, 0.05, BOX, x0=x0, seed=6, **KW), paths.calibrate(0.05, 0.05, BOX, x0=x0[:2], seed=6, **KW)
    for n in ('x', 'logp', 'accept_rate', 'step', 'status'):                     # a chain does not depend on the chains beside it
        assert np.array_equal(getattr(four, n)[:, :2], getattr(two, n)), n
    assert same(paths.calibrate(0.05, 0.05, BOX, x0=np.broadcast_to(x0, (6, 4, 2)).copy(), seed=6, **KW), four)


def test_gp_observation_and_prior(eng, gp_paths):
    from dgp_amd import calibrate
    m, paths = gp_paths
    y = 0.05 + 0.02 * np.random.default_rng(8).normal(size=(4, 1))               # T = 4 replicates at the same unknown x
    ybar = calibrate.observation(y, 0.1, 1)[0]
    rep, mean = paths.calibrate(y, 0.1, BOX, seed=2, **KW), paths.calibrate(ybar, 0.05, BOX, seed=2, **KW)
    assert same(rep, mean)
    gaps = paths.calibrate(np.concatenate([y, [[np.nan]]]), 0.1, BOX, seed=2, **KW)     # an unobserved entry is ignored
    assert same(gaps, rep)
    prior = (np.array([0.8, 0.2]), np.array([0.01, 0.01]))
    pulled = paths.calibrate(0.05, 0.05, BOX, seed=2, prior=prior, **KW)
    check_posterior(paths, pulled, 0.05, 0.05, 6, KW, prior)
    print('a strong prior: pooled mean %s' % pulled.pooled().mean(0))
    assert np.all(np.abs(pulled.pooled().mean(0) - prior[0]) < 0.03)
    half = paths.calibrate(0.05, 0.05, BOX, seed=2, prior=(prior[0], np.array([0.01, np.inf])), **KW)   # an infinite sd: flat
    assert abs(half.pooled()[:, 0].mean() - 0.8) < 0.03 and half.pooled()[:, 1].std() > 0.03


def test_gp_calibrate_entry_and_refusals(eng, gp_paths):
    from dgp_amd import gp, kernel
    m, paths = gp_paths
    np.random.seed(8)
    res = m.calibrate(0.05, 0.05, BOX, sample_size=5, n_features=64, seed=2, **SHORT)
    assert res.x.shape == (5, 4, 40, 2) and np.all(res.x >= 0.0) and np.all(res.x <= 1.0)
    np.random.seed(8)
    assert same(m.calibrate(0.05, 0.05, BOX, sample_size=5, n_features=64, seed=2, **SHORT), res)
    for bad in (BOX[0], BOX[:1], np.array([[0.0, 1.0], [np.nan, 1.0]]), np.array([[0.0, 1.0], [1.0, 0.5]]), BOX.T[:, :1]):
        with pytest.raises(ValueError):
            paths.calibrate(0.05, 0.05, bad, **SHORT)
    for kw in (dict(n_chains=0), dict(n_samples=0), dict(thin=0), dict(warmup=-1), dict(n_candidates=2), dict(x0=np.zeros((3, 4, 2))),
               dict(x0=np.zeros((4, 3))), dict(qmc=True, n_candidates=100), dict(scale=np.ones(3)), dict(prior=(np.zeros(2), np.zeros(2)))):
        with pytest.raises(ValueError):
            paths.calibrate(0.05, 0.05, BOX, **dict(SHORT, **kw))
    for y, sd in ((np.nan, 0.05), (np.zeros((2, 2)), 0.05), (0.05, 0.0), (0.05, -1.0), (0.05, np.ones(2))):
        with pytest.raises(ValueError):
            paths.calibrate(y, sd, BOX, **SHORT)
    np.random.seed(1)
    local = m.sample_functions_vecchia(sample_size=2, n_features=16, m=10)
    with pytest.raises(NotImplementedError, match='sample_functions '):
        local.calibrate(0.05, 0.05, BOX, **SHORT)
    X, Y = B.bowl()
    vg = gp(X, Y, kernel(length=np.array([0.5]), name='sexp'), vecchia=True, m=10)
    with pytest.raises(NotImplementedError):
        vg.calibrate(0.05, 0.05, BOX)


def test_emulator_calibrate(eng, emu_paths, monkeypatch):
    import copy
    from dgp_amd import calibrate, pathfun
    which, emu, paths = emu_paths
    y = float(np.median(B.values_of(paths, np.random.default_rng(1).uniform(size=(64, 2)))))    # a value the draws do take
    res = paths.calibrate(y, 0.05, BOX, seed=7, **SHORT)
    check_posterior(paths, res, y, 0.05, 6, SHORT)
    monkeypatch.setattr(calibrate, '_rounds_per_upload', lambda Q, Dx: 7)
    monkeypatch.setattr(pathfun, '_rows_per_call', lambda e, P, width: 64)
    assert same(paths.calibrate(y, 0.05, BOX, seed=7, **SHORT), res)
    monkeypatch.undo()
    state = copy.deepcopy(emu._sample_rng)
    fresh = emu.calibrate(y, 0.05, BOX, sample_size=2, n_features=64, seed=1, **SHORT)           # N = 2: four draws
    assert fresh.x.shape == (4, 4, 40, 2) and np.all(fresh.x >= 0.0) and np.all(fresh.x <= 1.0)
    emu._sample_rng = state
    assert same(emu.calibrate(y, 0.05, BOX, sample_size=2, n_features=64, seed=1, **SHORT), fresh)
    with pytest.raises(ValueError):
        paths.calibrate([y, y], 0.05, BOX, **SHORT)                              # one output
    with pytest.raises(ValueError):
        paths.calibrate(y, 0.05, BOX[:1], **SHORT)


def test_sampled_nodes_are_refused(eng):
    from dgp_amd import emulator
    X, model = T._model('hetero')
    emu = emulator(model.estimate(), N=2, seed=5)
    with pytest.raises(ValueError, match='sampled node'):
        emu.sample_functions(sample_size=2, n_features=16).calibrate(0.1, 0.1, np.array([[0.0, 1.0]]), **SHORT)
    with pytest.raises(ValueError, match='sampled node'):
        emu.calibrate(0.1, 0.1, np.array([[0.0, 1.0]]), sample_size=2, n_features=16, **SHORT)
    _, model = T._model('two-connect', 'sexp')
    emu = emulator(model.estimate(), N=2, seed=1)
    with pytest.raises(NotImplementedError, match='sample_functions '):
        emu.sample_functions_vecchia(sample_size=2, n_features=16, m=10).calibrate(0.1, 0.1, BOX, **SHORT)
