"""paths.calibrate(method='hmc') (dgp_amd/calibrate.py, DESIGN I.20) on the small models of tests/test_gpu_calibrate_model.py:
every draw's posterior against quadrature on a grid of the draw's own values, also where it presses on the walls of the box;
the log densities against paths(x); bit-for-bit replays and invariances; and method='mala' against a call without `method`.
Needs an MI355X: -m gpu.

As there, nothing compares trajectories with the restatement: the device's walk and numpy's differ in the last bits.  The 1-D
comparison is held on the CPU first (tests/test_boxhmc_host.py::test_line_case_on_the_cpu), which sets RHAT_MAX."""
import numpy as np
import pytest

import boxmala_ref as M
import test_boxmala_host as H
import test_gpu_boxmin_model as B
import test_gpu_calibrate_model as G
from test_gpu_calibrate_model import emu_paths, eng, gp_paths       # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu
MARGIN = 5.0
RHAT_MAX = 1.016      # (the CPU run's split R-hat lay in 0.9988 .. 1.0016: test_line_case_on_the_cpu; ten times its distance from 1)
LINE = dict(G.LINE, samples=400, warmup=200)
BOX = B.BOX
HMC = dict(method='hmc')
KW = dict(G.KW, **HMC)
SHORT = dict(G.SHORT, **HMC)


def evaluations(seed, kw, thin=1):
    from dgp_amd import calibrate
    return 1 + int(calibrate.trajectory_lengths(seed, kw['warmup'] + kw['n_samples'] * thin, kw.get('n_leapfrog', 8), kw.get('jitter', True)).sum())


def test_line_gp_against_quadrature(eng):
    """6 draws x 4 chains x 400 samples after 200 warm-up iterations, trajectories of 1 .. 8 steps: per draw the pooled mean
    and variance within 5 standard errors, by the samples' own ess, of their quadrature over paths(GRID); split R-hat below
    the CPU run's bound.  Observed on an MI355X (seed 1): z of the means 1.12, 1.43, 0.51, 0.43, 2.02, -1.22, of the variances
    0.62, -0.86, -0.60, -0.12, -2.34, -0.50; split R-hat at most 1.0014; ess 933 .. 1372 of 1600; acceptance 0.70 .. 0.89; 2611
    walk evaluations."""
    X, Y = G.line()
    m = G.T._gp('sexp', X, Y)
    np.random.seed(LINE['seed'])
    paths = m.sample_functions(sample_size=LINE['J'], n_features=LINE['F'])
    res = paths.calibrate(LINE['y'], LINE['sd'], G.BOX1, n_chains=LINE['chains'], n_samples=LINE['samples'], warmup=LINE['warmup'], seed=1, **HMC)
    assert res.x.shape == (6, 4, 400, 1) and np.all(res.status == 0) and (res.method, res.n_leapfrog) == ('hmc', 8)
    assert res.rounds == res.evaluations == evaluations(1, dict(warmup=200, n_samples=400))
    f_grid = paths(G.GRID[:, None])
    z = np.array([G.against_the_grid(res.x[p, :, :, 0], f_grid[:, p]) for p in range(LINE['J'])])
    print('line gp, hmc: acceptance %.2f .. %.2f, steps %.3g .. %.3g, ess %.0f .. %.0f of 1600, rhat max %.4f, %d evaluations' %
          (res.accept_rate.min(), res.accept_rate.max(), res.step.min(), res.step.max(), res.ess.min(), res.ess.max(), res.rhat.max(), res.evaluations))
    print('z of the means %s, of the variances %s' % (np.round(z[:, 0], 2), np.round(z[:, 1], 2)))
    assert np.max(np.abs(z)) <= MARGIN
    assert np.all(res.rhat < RHAT_MAX) and np.all(res.ess > 100)
    assert np.all(res.accept_rate > 0.5) and np.all(res.accept_rate < 0.98)


def test_gp_posterior_pressing_on_the_walls(eng, gp_paths):
    """The bowl (x0 - 0.3)^2 + (x1 - 0.6)^2 observed as y = 0 with sd 0.1: every draw's posterior is a plateau of radius about
    0.3 to 0.45 around (0.3, 0.6), which the walls x0 = 0 and x1 = 1 cut.  Per draw, against quadrature of paths(x) on a 201 x
    201 grid of the box: both means, and the share of the samples within 0.05 of the wall x0 = 0 (at least 2 % by
    quadrature), within 5 standard errors by the samples' own ess.  A sampler that lost or piled up mass at a wall would miss
    the share first.  Observed on an MI355X (seed 2): shares by quadrature 0.050 .. 0.063; z of the means of x0 -2.11 .. 0.15, of
    x1 -1.54 .. 1.14, of the share -0.17 .. 1.29; ess 628 .. 1443 of 2000; split R-hat at most 1.0061; acceptance 0.70 .. 0.89."""
    m, paths = gp_paths
    kw = dict(n_chains=4, n_samples=500, warmup=200, n_candidates=256, seed=2, **HMC)
    res = paths.calibrate(0.0, 0.1, BOX, **kw)
    assert np.all(res.x >= 0.0) and np.all(res.x <= 1.0) and np.all(res.status == 0)
    axis = np.linspace(0.0, 1.0, 201)
    mesh = np.stack(np.meshgrid(axis, axis, indexing='ij'), -1).reshape(-1, 2)
    f_grid = paths(mesh)                                                         # (201 * 201, 6)
    w, ybar = np.array([1.0 / 0.1 ** 2]), np.array([0.0])
    zs, shares = [], []
    for p in range(6):
        mean, _ = M.grid_posterior(f_grid[:, p].reshape(201, 201, 1), [axis, axis], ybar, w)
        lp = -0.5 * w[0] * f_grid[:, p].reshape(201, 201) ** 2
        wt = np.outer(M._trapezoid(axis), M._trapezoid(axis)) * np.exp(lp - lp.max())
        share = (wt[:10].sum() + 0.5 * wt[10].sum()) / wt.sum()                  # (node 10 lies on x0 = 0.05: half its weight)
        shares.append(share)
        x = res.x[p]
        zs.append([H.zscore(x[:, :, 0], mean[0]), H.zscore(x[:, :, 1], mean[1]), H.zscore((x[:, :, 0] <= axis[10]).astype(float), share)])
    print('bowl at the walls, hmc: acceptance %.2f .. %.2f, steps %.3g .. %.3g, ess %.0f .. %.0f of 2000, rhat max %.4f' %
          (res.accept_rate.min(), res.accept_rate.max(), res.step.min(), res.step.max(), res.ess.min(), res.ess.max(), res.rhat.max()))
    print('share within 0.05 of x0 = 0 by quadrature %s; z of the means %s, %s, of the share %s' %
          (np.round(shares, 3), np.round([z[0] for z in zs], 2), np.round([z[1] for z in zs], 2), np.round([z[2] for z in zs], 2)))
    assert min(shares) >= 0.02
    assert np.max(np.abs(zs)) <= MARGIN


def check_posterior(obj, res, y, sd, P, kw, seed):
    """test_gpu_calibrate_model.check_posterior for method='hmc': shapes, the box, the count of evaluations, and logp
    against the draws' own shared-rows evaluation within I.19's form bound."""
    R, S = kw['n_chains'], kw['n_samples']
    assert res.x.shape == (P, R, S, 2) and res.logp.shape == (P, R, S) and res.x0.shape == (P, R, 2)
    assert all(getattr(res, n).shape == (P, R) for n in ('accept_rate', 'step', 'status'))
    assert res.rounds == res.evaluations == evaluations(seed, kw) and (res.method, res.n_leapfrog) == ('hmc', 8)
    assert res.rhat.shape == (P, 2) and res.ess.shape == (P, 2) and res.pooled().shape == (P * R * S, 2)
    assert np.all(res.x >= BOX[:, 0]) and np.all(res.x <= BOX[:, 1]) and np.all(res.status == 0)
    assert np.all(res.accept_rate > 0.0) and np.all(res.step > 0.0)
    rows = res.x[:, :, -1].reshape(P * R, 2)
    own = np.repeat(np.arange(P), R)
    f = B.values_of(obj, rows)[np.arange(P * R), own]
    bound = B.form_bound(obj, rows)[np.arange(P * R), own]
    w = 1.0 / sd ** 2
    lp = -0.5 * w * (y - f) ** 2
    slack = w * np.abs(y - f) * bound + 0.5 * w * bound ** 2 + 16 * np.finfo(float).eps * np.abs(lp)
    diff = np.abs(res.logp[:, :, -1].reshape(-1) - lp)
    print('logp against paths(x): largest difference / bound %.3g' % np.max(diff / slack))
    assert np.all(diff <= slack)


def test_gp_calibrate(eng, gp_paths):
    m, paths = gp_paths
    res = paths.calibrate(0.05, 0.05, BOX, seed=3, **KW)
    check_posterior(paths, res, 0.05, 0.05, 6, KW, 3)
    assert G.same(res, paths.calibrate(0.05, 0.05, BOX, seed=3, **KW))           # the same arguments: the same bits
    assert not np.array_equal(res.x, paths.calibrate(0.05, 0.05, BOX, seed=4, **KW).x)
    r2 = np.sum((res.pooled() - np.array([0.3, 0.6])) ** 2, 1)                   # the ring of the bowl
    assert abs(np.median(r2) - 0.05) < 0.03
    fixed = paths.calibrate(0.05, 0.05, BOX, seed=3, n_leapfrog=3, jitter=False, **KW)
    assert fixed.evaluations == 1 + 3 * 200 and fixed.n_leapfrog == 3 and not np.array_equal(fixed.x, res.x)
    one = paths.calibrate(0.05, 0.05, BOX, seed=3, n_leapfrog=1, **KW)           # L = 1: a round per iteration, as MALA
    assert one.evaluations == 201 and np.all(one.x >= 0.0) and np.all(one.x <= 1.0)
    np.random.seed(8)
    entry = m.calibrate(0.05, 0.05, BOX, sample_size=5, n_features=64, seed=2, **SHORT)
    assert entry.x.shape == (5, 4, 40, 2) and entry.method == 'hmc'
    for bad in (dict(method='nuts'), dict(n_leapfrog=0)):
        with pytest.raises(ValueError):
            paths.calibrate(0.05, 0.05, BOX, **dict(SHORT, **bad))


def test_gp_blocks_and_starts_change_no_bit(eng, gp_paths, monkeypatch):
    from dgp_amd import calibrate, pathfun
    m, paths = gp_paths
    whole = paths.calibrate(0.05, 0.05, BOX, seed=5, **KW)
    for size in (1, 7, 64):
        monkeypatch.setattr(calibrate, '_rounds_per_upload', lambda Q, Dx, size=size: size)
        assert G.same(paths.calibrate(0.05, 0.05, BOX, seed=5, **KW), whole), size
    monkeypatch.undo()
    for rows in (7, 64, 200):
        monkeypatch.setattr(pathfun, '_rows_per_call', lambda e, P, width, rows=rows: rows)
        assert G.same(paths.calibrate(0.05, 0.05, BOX, seed=5, **KW), whole), rows
    monkeypatch.undo()
    x0 = np.random.default_rng(4).uniform(size=(4, 2))
    four, two = paths.calibrate(0.05, 0.05, BOX, x0=x0, seed=6, **KW), paths.calibrate(0.05, 0.05, BOX, x0=x0[:2], seed=6, **KW)
    for n in ('x', 'logp', 'accept_rate', 'step', 'status'):                     # a chain does not depend on the chains beside it
        assert np.array_equal(getattr(four, n)[:, :2], getattr(two, n)), n


def test_mala_is_what_it_was(eng, gp_paths):
    """method='mala' runs the code path of a call without `method`: the same bits, the same container."""
    m, paths = gp_paths
    old, new = paths.calibrate(0.05, 0.05, BOX, seed=3, **G.KW), paths.calibrate(0.05, 0.05, BOX, seed=3, method='mala', **G.KW)
    assert G.same(old, new) and (new.method, new.n_leapfrog, new.evaluations, new.rounds) == ('mala', 1, 201, 201)
    assert G.same(old, paths.calibrate(0.05, 0.05, BOX, seed=3, method='mala', n_leapfrog=3, jitter=False, target_accept=0.574, **G.KW))


def test_emulator_calibrate(eng, emu_paths, monkeypatch):
    from dgp_amd import calibrate, pathfun
    which, emu, paths = emu_paths
    y = float(np.median(B.values_of(paths, np.random.default_rng(1).uniform(size=(64, 2)))))    # a value the draws do take
    res = paths.calibrate(y, 0.05, BOX, seed=7, **SHORT)
    check_posterior(paths, res, y, 0.05, 6, SHORT, 7)
    assert G.same(paths.calibrate(y, 0.05, BOX, seed=7, **SHORT), res)
    monkeypatch.setattr(calibrate, '_rounds_per_upload', lambda Q, Dx: 7)
    monkeypatch.setattr(pathfun, '_rows_per_call', lambda e, P, width: 64)
    assert G.same(paths.calibrate(y, 0.05, BOX, seed=7, **SHORT), res)
    monkeypatch.undo()
    x0 = np.random.default_rng(4).uniform(size=(4, 2))
    four, two = paths.calibrate(y, 0.05, BOX, x0=x0, seed=6, **SHORT), paths.calibrate(y, 0.05, BOX, x0=x0[:2], seed=6, **SHORT)
    for n in ('x', 'logp', 'accept_rate', 'step', 'status'):
        assert np.array_equal(getattr(four, n)[:, :2], getattr(two, n)), n
    assert G.same(paths.calibrate(y, 0.05, BOX, seed=7, **G.SHORT), paths.calibrate(y, 0.05, BOX, seed=7, method='mala', **G.SHORT))
    fresh = emu.calibrate(y, 0.05, BOX, sample_size=2, n_features=64, seed=1, **SHORT)           # N = 2: four draws
    assert fresh.x.shape == (4, 4, 40, 2) and fresh.method == 'hmc' and np.all(fresh.x >= 0.0) and np.all(fresh.x <= 1.0)
