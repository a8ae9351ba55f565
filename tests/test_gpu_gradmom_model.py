"""paths.active_subspace(X) of gp models and emulators (dgp_amd/sensitivity.py, DESIGN I.18) on small models: the device sums
against the longdouble sums (tests/gradmom_ref.py) of the values and gradients that paths(X) and paths.grad(X) themselves
return at the same rows, the row blocks, columns the model does not read, the refusals, the convenience entries, and one
statistical check on a linear function.  Needs an MI355X: -m gpu."""
import numpy as np
import pytest

import gradmom_ref as R
import pathfun_ref as PR
import pathgrad_ref as GR
from test_gpu_pathfun import _model

pytestmark = pytest.mark.gpu
M_ROWS, F = 200, 64


@pytest.fixture(scope='module')
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    from dgp_amd.ops import default_engine
    return default_engine(0)


def rows(Dx, seed=1, n_rows=M_ROWS, bounds=None):
    from dgp_amd.sensitivity import uniform_design
    return uniform_design(np.array([[0.0, 1.0]] * Dx) if bounds is None else bounds, n_rows, seed=seed)


def host_values_and_jacobian(paths, X):
    """(f (P, M, K), J (P, M, K, Dx)) from paths(X) and paths.grad(X), in the kernel's layout."""
    out, grad = paths(X), paths.grad(X)
    if isinstance(out, np.ndarray):
        return out.T[:, :, None].copy(), grad.transpose(2, 0, 1)[:, :, None, :].copy()
    return np.stack([o.T for o in out], -1), np.stack([g.transpose(2, 0, 1) for g in grad], 2)


def check_against_evaluation(paths, X, what, bounds=None):
    """res.sums within the bound of the reference sums of the host copies, and C against the f64 einsum a user would write
    (which carries the same bound once more)."""
    res = paths.active_subspace(X, bounds)
    f, J = host_values_and_jacobian(paths, X)
    P, M, K, Dx = J.shape
    assert res.sums['sums'].shape == (P, K, R.n_sums(Dx)) and res.n_rows == M == len(X)
    assert np.array_equal(res.sums['shift'], f[:, 0, :])        # the values at row 0: the same bits at the same rows
    R.check(res.sums['sums'], f, J, res.sums['shift'], what)
    C = res.C if res.C.ndim == 4 else res.C[None]
    ein, mag = np.einsum('pmkd,pmke->kpde', J, J) / M, np.einsum('pmkd,pmke->kpde', np.abs(J), np.abs(J)) / M
    assert np.all(np.abs(C - ein) <= 2 * (M + 3) * R.U * mag)
    assert np.array_equal(C, C.transpose(0, 1, 3, 2))
    return res, f, J


def check_formulas(res, bounds, squeezed):
    ref = R.formulas(res.sums['sums'], res.sums['shift'], res.n_rows, bounds)
    for name in ('C', 'dgsm', 'mean_grad', 'mean', 'variance') + (() if bounds is None else ('total_bound',)):
        assert np.array_equal(getattr(res, name), ref[name][0] if squeezed else ref[name]), name
    assert np.all(ref['variance'] > 0)


def check_blocks(paths, X, res, monkeypatch):
    """Blocks of 64 rows (forced; 7 and 70 round to it) and of 192 against the one block the free memory gives: the same bits."""
    from dgp_amd import pathfun
    calls = []
    real = pathfun._row_blocks
    monkeypatch.setattr(pathfun, '_row_blocks', lambda *a, **kw: calls.append(1) or real(*a, **kw))
    for step in (64, 7, 70, 200):
        monkeypatch.setattr(pathfun, '_rows_per_call', lambda e, P, width: step)
        again = paths.active_subspace(X, res.bounds)
        assert all(np.array_equal(again.sums[k], res.sums[k]) for k in ('sums', 'shift')), step
        assert np.array_equal(again.C, res.C) and np.array_equal(again.eigenvalues, res.eigenvalues)
    assert len(calls) == 4
    monkeypatch.undo()


# ------------------------------------------------------------------------------------------------ gp
def _gp_two_of_three(kind='matern2.5', n=30):
    """A gp whose kernel reads columns {0, 2} of 3."""
    from dgp_amd import gp, kernel
    rng = np.random.default_rng(11)
    X = rng.uniform(size=(n, 3))
    Y = (np.sin(3 * X[:, 0]) + X[:, 2]**2)[:, None]
    return gp(X, Y, kernel(length=np.full(2, 0.7), name=kind, scale=1.9, nugget=1e-4, input_dim=np.array([0, 2])))


@pytest.mark.parametrize('kind', ['matern2.5', 'sexp'])
def test_gp_sums_formulas_blocks_and_the_unread_column(eng, kind, monkeypatch):
    m = _gp_two_of_three(kind)
    np.random.seed(21)
    paths = m.sample_functions(sample_size=4, n_features=F)
    X = rows(3)
    bounds = np.array([[0.0, 1.0]] * 3)
    res, f, J = check_against_evaluation(paths, X, 'gp ' + kind, bounds)
    assert res.C.shape == (4, 3, 3) and res.dgsm.shape == res.total_bound.shape == (3, 4) and res.eigenvalues.shape == (4, 3)
    check_formulas(res, bounds, True)
    check_blocks(paths, X, res, monkeypatch)
    # the column the kernel does not read: exactly +0 in its sum, its row and its column
    assert np.all(res.C[:, 1, :] == 0.0) and np.all(res.C[:, :, 1] == 0.0) and not np.any(np.signbit(res.C[:, 1, :]))
    assert np.all(res.mean_grad[1] == 0.0) and np.all(res.dgsm[1] == 0.0) and np.all(res.total_bound[1] == 0.0)
    assert np.all(res.dgsm[[0, 2]] > 0.0) and np.all(res.eigenvalues[:, 2] <= 1e-14 * res.eigenvalues[:, 0])
    s = res.summary()
    assert s['dgsm']['mean'].shape == s['total_bound']['upper'].shape == (3,)


def test_gp_convenience(eng):
    """gp.active_subspace draws the functions, makes the design and calls paths.active_subspace: the same result from the
    same generator states."""
    from dgp_amd.sensitivity import ActiveSubspaceResult
    m = _gp_two_of_three()
    bounds = np.array([[0.0, 1.0], [-1.0, 1.0], [0.0, 2.0]])
    np.random.seed(5)
    res = m.active_subspace(bounds, n_rows=256, sample_size=4, n_features=F, seed=1)
    assert isinstance(res, ActiveSubspaceResult) and res.n_rows == 256 and res.C.shape == (4, 3, 3)
    assert np.array_equal(res.bounds, bounds) and np.array_equal(res.scale, [0.5, 1.0, 1.0])
    np.random.seed(5)
    ref = m.sample_functions(sample_size=4, n_features=F).active_subspace(rows(3, seed=1, n_rows=256, bounds=bounds), bounds)
    assert np.array_equal(res.sums['sums'], ref.sums['sums']) and np.array_equal(res.eigenvectors, ref.eigenvectors)
    np.random.seed(5)
    q = m.active_subspace(bounds, n_rows=256, sample_size=4, n_features=F, seed=1, qmc=True)
    assert q.C.shape == (4, 3, 3) and not np.array_equal(q.C, res.C)


# ------------------------------------------------------------------------------------------------ emulators
def _two_layer(n=40):
    """Two hidden nodes that read the three columns of x, one output node on top of them."""
    from dgp_amd import dgp, kernel, combine
    rng = np.random.default_rng(6)
    K = lambda **kw: kernel(length=np.array([1.0]), name='matern2.5', nugget=1e-4, **kw)
    X = rng.uniform(size=(n, 3))
    Y = np.sin(4 * X[:, :1]) * np.cos(2 * X[:, 1:2]) + X[:, 2:]**2 + 0.02 * rng.normal(size=(n, 1))
    model = dgp(X, Y, combine([K(), K()], [K(scale_est=True)]), seed=4)
    model.train(N=3, ess_burn=3, disable=True)
    return X, model


@pytest.fixture(scope='module')
def emu(eng):
    from dgp_amd import emulator
    X, model = _two_layer()
    return emulator(model.estimate(), N=2, seed=5)


def test_emulator_sums_formulas_blocks(eng, emu, monkeypatch):
    paths = emu.sample_functions(sample_size=3, n_features=F)
    X = rows(3)
    res, f, J = check_against_evaluation(paths, X, 'two-layer emulator')
    assert res.C.shape == (1, 6, 3, 3) and res.dgsm.shape == res.mean_grad.shape == (1, 3, 6) and res.variance.shape == (1, 6)
    check_formulas(res, None, False)
    check_blocks(paths, X, res, monkeypatch)
    assert np.all(res.dgsm > 0.0)
    W, dist = res.subspace(1)
    assert W.shape == (3, 1) and dist.shape == (6,) and np.all((dist >= 0.0) & (dist <= 1.0 + 1e-12))
    with pytest.raises(ValueError, match='bounds'):
        res.total_bound


def test_emulator_extra_column_is_exactly_zero(eng, emu):
    paths = emu.sample_functions(sample_size=3, n_features=F)
    res, f, J = check_against_evaluation(paths, rows(4), 'two-layer emulator with an extra column')
    assert res.C.shape == (1, 6, 4, 4)
    assert np.all(res.C[:, :, 3, :] == 0.0) and np.all(res.C[:, :, :, 3] == 0.0) and np.all(res.mean_grad[:, 3] == 0.0)
    z = res.sums['sums'][..., 2 + 3]
    assert np.all(z == 0.0) and not np.any(np.signbit(z))
    assert np.all(res.dgsm[:, :3] > 0.0)


def test_emulator_convenience(eng, emu):
    """emulator.active_subspace against sample_functions + uniform_design + paths.active_subspace from an equal generator
    state."""
    from dgp_amd.sensitivity import ActiveSubspaceResult, uniform_design
    bounds = np.array([[0.0, 1.0], [0.0, 0.5], [0.2, 1.0]])
    state = emu._sample_rng.bit_generator.state
    res = emu.active_subspace(bounds, n_rows=256, seed=1, sample_size=3, n_features=F)
    assert isinstance(res, ActiveSubspaceResult) and res.n_rows == 256 and res.C.shape == (1, 6, 3, 3)
    assert res.total_bound.shape == (1, 3, 6) and np.all(np.isfinite(res.total_bound))
    emu._sample_rng.bit_generator.state = state
    ref = emu.sample_functions(sample_size=3, n_features=F).active_subspace(uniform_design(bounds, 256, seed=1), bounds)
    assert np.array_equal(res.sums['sums'], ref.sums['sums']) and np.array_equal(res.sums['shift'], ref.sums['shift'])
    assert np.array_equal(res.eigenvalues, ref.eigenvalues) and np.array_equal(res.total_bound, ref.total_bound)


def test_refusals(eng, emu):
    from dgp_amd import emulator
    bounds = np.array([[0.0, 1.0]] * 3)
    X, model = _model('hetero')
    het = emulator(model.estimate(), N=2, seed=5)
    with pytest.raises(ValueError, match='has no derivative'):
        het.active_subspace(bounds[:1], n_rows=64, sample_size=2, n_features=16)
    with pytest.raises(ValueError, match='has no derivative'):
        het.sample_functions(sample_size=2, n_features=16).active_subspace(rows(1, n_rows=64))
    with pytest.raises(NotImplementedError, match='active_subspace: a draw made by local conditioning'):
        emu.sample_functions_vecchia(sample_size=2, n_features=16, m=10).active_subspace(rows(3, n_rows=64))
    m = _gp_two_of_three()
    with pytest.raises(NotImplementedError, match='active_subspace: a draw made by local conditioning'):
        m.sample_functions_vecchia(sample_size=2, n_features=16, m=10).active_subspace(rows(3, n_rows=64))
    paths = m.sample_functions(sample_size=2, n_features=16)
    with pytest.raises(ValueError, match='the model reads column 2'):
        paths.active_subspace(rows(2, n_rows=64))
    with pytest.raises(ValueError, match='at least 2 rows'):
        paths.active_subspace(rows(3, n_rows=1))


# ------------------------------------------------------------------------------------------------ one statistical check
STAT_A = np.array([1.0, 2.0, -0.5])
STAT_BOUNDS = np.array([[0.0, 1.0], [0.0, 2.0], [-1.0, 1.0]])
STAT_SEED, STAT_J, STAT_F, STAT_ROWS, STAT_BASE, STAT_BATCHES = 17, 4, 256, 16384, 16384, 16
STAT_KIND, STAT_LENGTH, STAT_SCALE, STAT_NUGGET = 'sexp', np.full(3, 3.0), 4.0, 1e-6
STAT_ALIGNMENT = 0.999         # the threshold on |w . S a| / |S a|; test_gradmom_host.py holds it to the restatement's margin


def stat_data():
    """y = a . x at 40 rows of the box."""
    X = STAT_BOUNDS[:, 0] + (STAT_BOUNDS[:, 1] - STAT_BOUNDS[:, 0]) * np.random.default_rng(31).uniform(size=(40, 3))
    return X, (X @ STAT_A)[:, None]


def stat_designs():
    from dgp_amd.sensitivity import saltelli_design, uniform_design
    return uniform_design(STAT_BOUNDS, STAT_ROWS, seed=2), saltelli_design(STAT_BOUNDS, STAT_BASE, seed=3)


def stat_restated():
    """The statistical check on the numpy restatement (tests/pathfun_ref.py, tests/pathgrad_ref.py) with the generator draws
    of gp.sample_functions under np.random.seed(STAT_SEED) in their documented order.  No device.  Returns
    (alignment (J + 1,) of every draw and of the mean over the draws, its standard error, margin (Dx, J) = total_bound - total,
    its standard error): the standard
    errors from STAT_BATCHES batches of consecutive rows, sd of the batch statistics / sqrt(STAT_BATCHES)."""
    from dgp_amd import pathfun
    W, Y = stat_data()
    np.random.seed(STAT_SEED)
    Omega, b = pathfun.features(np.random, STAT_KIND, STAT_LENGTH, 3, STAT_F)
    theta, eps = np.random.standard_normal((STAT_J, STAT_F)), np.random.standard_normal((STAT_J, len(W)))
    v = PR.weights(W, Y[:, 0], Omega, b, theta, eps, STAT_KIND, STAT_LENGTH, STAT_SCALE, STAT_NUGGET, None)
    X, (A, B) = stat_designs()
    args = (W, Omega, b, theta, v, STAT_KIND, STAT_LENGTH, STAT_SCALE)
    f, G = PR.evaluate(X, *args), GR.grad(X, *args)                         # (J, M), (J, M, 3)
    fA, fB = PR.evaluate(A, *args), PR.evaluate(B, *args)
    fAB = []
    for i in range(3):
        AB = A.copy()
        AB[:, i] = B[:, i]
        fAB.append(PR.evaluate(AB, *args))
    scale, width = 0.5 * (STAT_BOUNDS[:, 1] - STAT_BOUNDS[:, 0]), STAT_BOUNDS[:, 1] - STAT_BOUNDS[:, 0]
    lead = scale * STAT_A / np.linalg.norm(scale * STAT_A)

    def statistics(r, q):
        """From the rows r of X and q of (A, B): (alignment (J + 1,) of every draw and of the mean over draws, margin (Dx, J))."""
        C = np.einsum('pmd,pme->pde', G[:, r], G[:, r]) / len(r)
        scaled = C * scale[:, None] * scale[None, :]
        w = np.linalg.eigh(np.concatenate((scaled, scaled.mean(0)[None])))[1][:, :, -1]
        bound = np.einsum('pdd->dp', C) * (width**2)[:, None] / (np.pi**2 * f[:, r].var(1))
        VAB = np.concatenate((fA[:, q], fB[:, q]), 1).var(1)
        total = np.stack([((fA[:, q] - fi[:, q])**2).mean(1) / (2 * VAB) for fi in fAB])
        return np.abs(w @ lead), bound - total
    align, margin = statistics(np.arange(STAT_ROWS), np.arange(STAT_BASE))
    batches = [statistics(r, q) for r, q in zip(np.split(np.arange(STAT_ROWS), STAT_BATCHES), np.split(np.arange(STAT_BASE), STAT_BATCHES))]
    se = [np.std([bt[i] for bt in batches], axis=0, ddof=1) / np.sqrt(STAT_BATCHES) for i in range(2)]
    return align, se[0], margin, se[1]


def test_a_linear_function_has_one_direction_and_the_bound_holds(eng):
    """4 draws (256 features) of a gp on y = a . x over a box with unequal sides, fixed hyperparameters, 16384 rows: the
    leading direction of subspace(1) against S a / |S a|, and total_bound against paths.sobol's total index, input by input
    and draw by draw.  For a linear function the bound exceeds the index by the factor 12 / pi^2 = 1.216.  Both margins were
    taken on the numpy restatement first (stat_restated, held to it by tests/test_gradmom_host.py): the alignment there is
    0.999976 for the worst draw with standard errors below 5e-7, so the threshold 0.999 lies more than two thousand standard
    errors below it; the smallest margin of the bound over its index is 19.3 standard errors (DESIGN I.18)."""
    from dgp_amd import gp, kernel
    X, Y = stat_data()
    m = gp(X, Y, kernel(length=STAT_LENGTH.copy(), name=STAT_KIND, scale=STAT_SCALE, nugget=STAT_NUGGET))
    np.random.seed(STAT_SEED)
    paths = m.sample_functions(sample_size=STAT_J, n_features=STAT_F)
    Xd, (A, B) = stat_designs()
    res = paths.active_subspace(Xd, STAT_BOUNDS)
    W, dist = res.subspace(1)
    lead = res.scale * STAT_A / np.linalg.norm(res.scale * STAT_A)
    align = abs(W[:, 0] @ lead)
    total = paths.sobol(A, B).total
    print('alignment %.9f (threshold %g); draws at distance <= %.3g; min (total_bound - total) / total = %.4f'
          % (align, STAT_ALIGNMENT, dist.max(), ((res.total_bound - total) / total).min()))
    assert align >= STAT_ALIGNMENT
    assert np.all(np.abs(res.eigenvectors[:, :, 0] @ lead) >= STAT_ALIGNMENT)
    assert np.all(res.total_bound >= total)
