"""paths.sobol(A, B) of gp models and emulators (dgp_amd/sensitivity.py, DESIGN I.16) on small models: the device sums against
the exact sums (tests/sobol_ref.py) of the values that paths(x) itself returns at the same rows, the indices as a bit-for-bit
replay of the formulas, the row blocks, columns the model does not read, the Vecchia paths, the refusals, and one statistical
check against analytic indices.  Needs an MI355X: -m gpu."""
import numpy as np
import pytest

import pathfun_ref as PR
import sobol_ref as R
from test_gpu_pathfun import _gp, _model

pytestmark = pytest.mark.gpu
N_BASE, F, J = 300, 200, 3
NTILES = -(-N_BASE // 64)


@pytest.fixture(scope='module')
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    from dgp_amd.ops import default_engine
    return default_engine(0)


def design(Dx, seed=1, n_base=N_BASE):
    from dgp_amd.sensitivity import saltelli_design
    return saltelli_design(np.array([[0.0, 1.0]] * Dx), n_base, seed=seed)


def stacked(A, B):
    """[A, B, AB_1, ..., AB_D]: the rows a user evaluates without sobol."""
    out = [A, B]
    for i in range(A.shape[1]):
        AB = A.copy()
        AB[:, i] = B[:, i]
        out.append(AB)
    return np.vstack(out)


def values_at(paths, x, n_base):
    """(2 + Dx, P, n_base, K): paths(x) at the stacked design, in the kernels' layout."""
    out = paths(x)
    f = out.T[:, :, None] if isinstance(out, np.ndarray) else np.stack([o.T for o in out], -1)      # (P, M, K)
    return f.reshape(f.shape[0], -1, n_base, f.shape[2]).transpose(1, 0, 2, 3)


def check_against_evaluation(paths, A, B, what):
    res = paths.sobol(A, B)
    f = values_at(paths, stacked(A, B), len(A))
    Dx, P, K = A.shape[1], f.shape[1], f.shape[3]
    s = res.sums
    assert s['base'].shape == (P, K, 4) and s['pair'].shape == (Dx, P, K, 2) and res.n_base == len(A)
    assert np.array_equal(s['shift'], f[0][:, 0, :])            # f_A at row 0 of the whole design: the same bits at the same rows
    R.check(s['base'], *R.exact_sums(f[0], f[1], None, s['shift']), NTILES, what + ' base')
    for i in range(Dx):
        R.check(s['pair'][i], *R.exact_sums(f[0], f[1], f[2 + i], s['shift']), NTILES, what + ' pair %d' % i)
    return res


def check_formulas(res, squeezed):
    first, total, V = R.indices(res.sums['base'], res.sums['pair'], res.n_base)
    mean = res.sums['shift'] + (res.sums['base'][..., 0] + res.sums['base'][..., 1]) / (2 * res.n_base)
    first, total, V, mean = first.transpose(2, 0, 1), total.transpose(2, 0, 1), V.T, mean.T
    if squeezed:
        first, total, V, mean = first[0], total[0], V[0], mean[0]
    assert np.all(V > 0)
    assert np.array_equal(res.first, first) and np.array_equal(res.total, total)
    assert np.array_equal(res.variance, V) and np.array_equal(res.mean, mean)


def check_blocks(paths, A, B, res, monkeypatch):
    from dgp_amd import pathfun
    for step in (7, 64, 70, 200):
        monkeypatch.setattr(pathfun, '_rows_per_call', lambda e, P, width: step)
        again = paths.sobol(A, B)
        assert all(np.array_equal(again.sums[k], res.sums[k]) for k in ('base', 'pair', 'shift')), step
        assert np.array_equal(again.first, res.first) and np.array_equal(again.total, res.total)
    monkeypatch.undo()


# ------------------------------------------------------------------------------------------------ gp
def _gp_two_of_three(kind='matern2.5'):
    """A gp whose kernel reads columns {0, 2} of 3."""
    from dgp_amd import gp, kernel
    rng = np.random.default_rng(11)
    X = rng.uniform(size=(50, 3))
    Y = (np.sin(3 * X[:, 0]) + X[:, 2]**2)[:, None]
    return gp(X, Y, kernel(length=np.full(2, 0.7), name=kind, scale=1.9, nugget=1e-4, input_dim=np.array([0, 2])))


@pytest.mark.parametrize('kind', ['matern2.5', 'sexp'])
def test_gp_sums_formulas_blocks(eng, kind, monkeypatch):
    rng = np.random.default_rng(11)
    X = rng.uniform(size=(60, 3))
    Y = (np.sin(3 * X[:, 0]) + X[:, 1] * X[:, 2] + 0.05 * rng.normal(size=len(X)))[:, None]
    m = _gp(kind, X, Y, connect=np.array([2]))
    np.random.seed(21)
    paths = m.sample_functions(sample_size=J, n_features=F)
    A, B = design(3)
    res = check_against_evaluation(paths, A, B, 'gp ' + kind)
    assert res.first.shape == res.total.shape == (3, J) and res.variance.shape == res.mean.shape == (J,)
    check_formulas(res, True)
    check_blocks(paths, A, B, res, monkeypatch)
    s = res.summary()
    assert s['first']['mean'].shape == s['total']['upper'].shape == (3,)


def test_gp_unread_column_is_exactly_zero(eng):
    m = _gp_two_of_three()
    np.random.seed(3)
    paths = m.sample_functions(sample_size=J, n_features=F)
    A, B = design(3)
    res = check_against_evaluation(paths, A, B, 'gp reading columns 0 and 2')
    assert np.all(res.sums['pair'][1] == 0.0) and np.all(res.first[1] == 0.0) and np.all(res.total[1] == 0.0)
    assert np.all(res.total[[0, 2]] > 0.0)


def test_gp_convenience(eng):
    """gp.sobol draws the functions, makes the design and calls paths.sobol: the same result from the same generator states."""
    from dgp_amd.sensitivity import SobolResult
    m = _gp_two_of_three()
    bounds = np.array([[0.0, 1.0]] * 3)
    np.random.seed(5)
    res = m.sobol(bounds, n_base=128, sample_size=J, n_features=F, seed=9)
    assert isinstance(res, SobolResult) and res.n_base == 128 and res.first.shape == (3, J)
    np.random.seed(5)
    A, B = design(3, seed=9, n_base=128)
    ref = m.sample_functions(sample_size=J, n_features=F).sobol(A, B)
    assert np.array_equal(res.first, ref.first) and np.array_equal(res.total, ref.total)
    np.random.seed(5)
    q = m.sobol(bounds, n_base=128, sample_size=J, n_features=F, seed=9, qmc=True)
    assert q.first.shape == (3, J) and not np.array_equal(q.first, res.first)


# ------------------------------------------------------------------------------------------------ emulators
@pytest.fixture(scope='module')
def emulators(eng):
    from dgp_amd import emulator
    out = {}
    for which in ('two-connect', 'three'):
        X, model = _model(which)
        out[which] = X, emulator(model.estimate(), N=2, seed=5)
    return out


@pytest.mark.parametrize('which', ['two-connect', 'three'])
def test_emulator_sums_formulas_blocks(eng, emulators, which, monkeypatch):
    X, emu = emulators[which]
    paths = emu.sample_functions(sample_size=J, n_features=F)
    A, B = design(X.shape[1])
    res = check_against_evaluation(paths, A, B, which)
    assert res.first.shape == res.total.shape == (1, X.shape[1], 2 * J) and res.variance.shape == res.mean.shape == (1, 2 * J)
    check_formulas(res, False)
    check_blocks(paths, A, B, res, monkeypatch)


def test_emulator_extra_column_is_exactly_zero(eng, emulators):
    X, emu = emulators['two-connect']
    paths = emu.sample_functions(sample_size=J, n_features=F)
    A, B = design(X.shape[1] + 1)
    res = check_against_evaluation(paths, A, B, 'two-connect with an extra column')
    assert res.first.shape == (1, 3, 2 * J)
    assert np.all(res.sums['pair'][2] == 0.0) and np.all(res.first[:, 2] == 0.0) and np.all(res.total[:, 2] == 0.0)
    assert np.all(res.total[:, :2] > 0.0)


def test_vecchia_paths(eng, monkeypatch):
    """The three checks on sample_functions_vecchia(m=20) paths of a model after to_vecchia(), and the convenience on it."""
    from dgp_amd import emulator
    X, model = _model('two-connect')
    emu = emulator(model.estimate(), N=2, seed=5)
    emu.to_vecchia()
    paths = emu.sample_functions_vecchia(sample_size=J, n_features=F, m=20)
    A, B = design(X.shape[1])
    res = check_against_evaluation(paths, A, B, 'vecchia two-connect')
    check_formulas(res, False)
    check_blocks(paths, A, B, res, monkeypatch)
    conv = emu.sobol(np.array([[0.0, 1.0]] * 2), n_base=128, sample_size=2, n_features=64, seed=1, m=20)
    assert conv.first.shape == (1, 2, 4) and np.all(np.isfinite(conv.first))


def test_refusals(eng, emulators):
    from dgp_amd import emulator
    bounds = np.array([[0.0, 1.0]] * 2)
    for which in ('hetero', 'categorical'):
        X, model = _model(which)
        emu = emulator(model.estimate(), N=2, seed=5)
        with pytest.raises(ValueError, match='drawn afresh on every evaluation'):
            emu.sobol(bounds[:X.shape[1]], n_base=64, sample_size=2, n_features=16)
        A, B = design(X.shape[1])
        with pytest.raises(ValueError, match='drawn afresh on every evaluation'):
            emu.sample_functions(sample_size=2, n_features=16).sobol(A, B)
    X, emu = emulators['two-connect']
    emu.shard = True
    try:
        with pytest.raises(NotImplementedError, match='sharded over ranks'):
            emu.sobol(bounds, n_base=64, sample_size=2, n_features=16)
    finally:
        emu.shard = False
    paths = emu.sample_functions(sample_size=2, n_features=16)
    A, B = design(2)
    with pytest.raises(Exception, match='2d-array'):
        paths.sobol(A[0], B[0])
    with pytest.raises(ValueError, match='n_base must be at least 2'):
        paths.sobol(A[:1], B[:1])


# ------------------------------------------------------------------------------------------------ one statistical check
STAT_ANALYTIC = np.array([0.2, 0.8, 0.0])
STAT_SEED, STAT_J, STAT_F, STAT_BASE = 17, 20, 512, 2048
STAT_KIND, STAT_LENGTH, STAT_SCALE, STAT_NUGGET = 'matern2.5', np.full(3, 2.0), 4.0, 1e-5


def stat_data():
    """y = x0 + 2 x1 at 50 rows of [0, 1]^3, the third column inert (read by the kernel, absent from y): Var y = 1/12 + 4/12, the
    first-order indices 1/5, 4/5, 0."""
    X = np.random.default_rng(31).uniform(size=(50, 3))
    return X, (X[:, 0] + 2.0 * X[:, 1])[:, None]


def stat_restated():
    """The draw-averaged first-order indices of the numpy restatement (tests/pathfun_ref.py) with the generator draws of
    gp.sample_functions under np.random.seed(STAT_SEED) in their documented order, by the reference estimator.  No device."""
    from dgp_amd import pathfun
    W, Y = stat_data()
    np.random.seed(STAT_SEED)
    Omega, b = pathfun.features(np.random, STAT_KIND, STAT_LENGTH, 3, STAT_F)
    theta, eps = np.random.standard_normal((STAT_J, STAT_F)), np.random.standard_normal((STAT_J, len(W)))
    v = PR.weights(W, Y[:, 0], Omega, b, theta, eps, STAT_KIND, STAT_LENGTH, STAT_SCALE, STAT_NUGGET, None)
    A, B = design(3, seed=2, n_base=STAT_BASE)
    f = PR.evaluate(stacked(A, B), W, Omega, b, theta, v, STAT_KIND, STAT_LENGTH, STAT_SCALE).reshape(STAT_J, 5, STAT_BASE)
    g = f - f[:, :1, :1]
    base = np.stack([g[:, 0].sum(1), g[:, 1].sum(1), (g[:, 0]**2).sum(1), (g[:, 1]**2).sum(1)], -1)
    pair = np.stack([np.stack([(g[:, 1] * (g[:, 2 + i] - g[:, 0])).sum(1), ((g[:, 0] - g[:, 2 + i])**2).sum(1)], -1) for i in range(3)])
    return R.indices(base, pair, STAT_BASE)[0].mean(-1)
    g = f - f[:, :1, :1]
    base = np.stack([g[:, 0].sum(1), g[:, 1].sum(1), (g[:, 0]**2).sum(1), (g[:, 1]**2).sum(1)], -1)
    pair = np.stack([np.stack([(g[:, 1] * (g[:, 2 + i] - g[:, 0])).sum(1), ((g[:, 0] - g[:, 2 + i])**2).sum(1)], -1) for i in range(3)])
    return R.indices(base, pair, STAT_BASE)[0].mean(-1)


STAT_CPU_DEVIATION = 0.0368042      # max_i |stat_restated()_i - analytic_i| (tests/test_sobol_host.py holds it to the restatement)


def test_draw_averaged_indices_are_the_analytic_ones(eng):
    """20 draws (512 features) of a gp on y = x0 + 2 x1 with fixed hyperparameters, n_base = 2048: the draw-averaged first-order
    indices against 1/5, 4/5, 0.  The tolerance is measured, not chosen: the numpy restatement with the same generator draws
    and the reference estimator (stat_restated, no device) gives 0.195257, 0.763196, 0.0000246 -- deviations 0.00474, 0.03680,
    0.0000246 from the analytic values, one realisation of the same emulation error (50 training rows, 512 features) and
    Monte-Carlo error (2048 base rows, 20 draws).  Tolerance: twice its largest deviation, 2 * 0.0368042 = 0.0736084, on the
    largest deviation of the device's averages."""
    from dgp_amd import gp, kernel
    X, Y = stat_data()
    m = gp(X, Y, kernel(length=STAT_LENGTH.copy(), name=STAT_KIND, scale=STAT_SCALE, nugget=STAT_NUGGET))
    np.random.seed(STAT_SEED)
    paths = m.sample_functions(sample_size=STAT_J, n_features=STAT_F)
    res = paths.sobol(*design(3, seed=2, n_base=STAT_BASE))
    mean = res.first.mean(-1)
    dev = np.abs(mean - STAT_ANALYTIC)
    print('draw-averaged first-order indices %s: deviations %s (tolerance %.6g)' % (mean, dev, 2 * STAT_CPU_DEVIATION))
    assert dev.max() <= 2 * STAT_CPU_DEVIATION
    assert np.array_equal(res.summary()['first']['mean'], mean)
