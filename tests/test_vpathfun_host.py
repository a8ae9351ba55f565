"""Host-side checks of function-valued draws by local conditioning (no GPU; DESIGN I.14): the public signatures and the
declared entry, and the numpy restatement (tests/vpathfun_ref.py) that the GPU tests compare the device against -- its mean is
the oracle's gp_vecch, its variance tends to gp_vecch's, and with every training row in the set it is pathfun_ref's dense
update."""
import inspect

import numpy as np
import pytest

from test_pathfun_host import F_BIG, feature_bound


def model(kind, nlen, seed=3):
    """n = 70, D = 3, m = 12, replicate weights: (W, y, omega, x, length, scale, nugget, m)."""
    rng = np.random.default_rng(seed)
    n, D, M = 70, 3, 15
    W, x = rng.uniform(size=(n, D)), rng.uniform(size=(M, D))
    x[0] = W[5]   # a row lying on a training row
    y = np.sin(4 * W[:, 0]) + W[:, 1] ** 2 + 0.1 * rng.normal(size=n)
    omega = 1.0 / rng.integers(1, 4, size=n)
    length = np.array([0.8]) if nlen == 'one' else np.array([0.6, 1.1, 0.9])
    return W, y, omega, x, length, 1.7, 1e-3, 12


def test_signatures_and_entry():
    from dgp_amd import _lib, emulator, gp, ops, vpathfun
    for cls in (emulator, gp):
        p = inspect.signature(cls.sample_functions_vecchia).parameters
        assert list(p) == ['self', 'sample_size', 'n_features', 'm']
        assert (p['sample_size'].default, p['n_features'].default, p['m'].default) == (50, 2048, 50)
    assert len(_lib.SIGNATURES['dgpamd_vpathfun_update'][1]) == 20
    assert list(inspect.signature(ops.Engine.vpathfun_update).parameters)[:10] == \
        ['self', 'kind', 'x', 'w', 'NN', 'r', 'prior', 'scale', 'nugget', 'jitters']
    assert vpathfun.LADDER == (0.0, 1e-10, 1e-8)
    for name in ('__call__', 'noise_sd', 'value_and_grad', 'build_shared', 'build_per_group'):
        assert hasattr(vpathfun.VecchiaNodePaths, name)


def test_m_below_one_is_refused_before_anything_else():
    """In vpaths.check_args' words, before the model is looked at (the emulator's refusal: tests/test_gpu_vpathfun_model.py)."""
    from dgp_amd import gp
    with pytest.raises(ValueError, match='sample_paths_vecchia: the conditioning-set size m must be at least 1'):
        gp.sample_functions_vecchia(object.__new__(gp), m=0)


@pytest.mark.parametrize('nlen', ['one', 'D'])
@pytest.mark.parametrize('kind', ['sexp', 'matern2.5'])
def test_restatement_correlation_is_the_oracles(kind, nlen):
    from oracle import dgp_oracle as O
    import vpathfun_ref as V
    W, _, _, x, length, _, _, _ = model(kind, nlen)
    got = V.corr((W / length)[:, None, :] - (x / length)[None, :, :], kind)
    np.testing.assert_allclose(got, O.cross_corr(W, x, length, kind), rtol=1e-13, atol=0)


@pytest.mark.parametrize('nlen', ['one', 'D'])
@pytest.mark.parametrize('kind', ['sexp', 'matern2.5'])
def test_mean_is_gp_vecch(kind, nlen):
    """theta = 0, eps = 0: r = y / sqrt(s) and the path is gp_vecch's mean on the oracle's own conditioning sets, at
    test_oracle_golden's tolerances for that function."""
    from oracle import dgp_oracle as O
    import vpathfun_ref as V
    W, y, omega, x, length, scale, nugget, m = model(kind, nlen)
    F = 8
    Omega, b = np.random.default_rng(1).normal(size=(F, 3)), np.zeros(F)
    r = (y / np.sqrt(scale))[None]
    got = V.evaluate(x, W, Omega, b, np.zeros((1, F)), r, kind, length, scale, nugget, m, omega)[0]
    NN = O.pred_nn(x / length, W / length, m)
    assert np.array_equal(NN, V.neighbours(x / length, W / length, m))
    want, _ = O.gp_vecch(x, W, NN, y, scale, length, nugget, omega, kind)
    np.testing.assert_allclose(got, want, rtol=1e-8, atol=1e-10)


@pytest.mark.parametrize('nlen', ['one', 'D'])
@pytest.mark.parametrize('kind', ['sexp', 'matern2.5'])
def test_variance_tends_to_gp_vecch(kind, nlen):
    """Given the features the variance over (theta, eps) is s ([1, -b] Phi Phi^T [1, -b]^T + eta b^T diag(omega) b); at
    F = 65536 it lies within I.12's (1 + |b|_1)^2 6 sqrt(1.5 / F) s of s (1 - a^T A_N^-1 a), gp_vecch's variance less the
    s eta that noise=True adds back."""
    from dgp_amd import pathfun
    from oracle import dgp_oracle as O
    import vpathfun_ref as V
    W, y, omega, x, length, scale, nugget, m = model(kind, nlen)
    Omega, b = pathfun.features(np.random.default_rng(2024), kind, length, 3, F_BIG)
    var, limit, l1 = V.variance(x, W, Omega, b, kind, length, scale, nugget, m, omega)
    _, vref = O.gp_vecch(x, W, O.pred_nn(x / length, W / length, m), y, scale, length, nugget, omega, kind)
    np.testing.assert_allclose(limit, vref - scale * nugget, rtol=1e-8, atol=1e-10)
    bound = (1.0 + l1) ** 2 * feature_bound(F_BIG) * scale
    print('kind %s, lengths %s: max |var - limit| / bound = %.3g' % (kind, nlen, (np.abs(var - limit) / bound).max()))
    assert np.all(np.abs(var - limit) <= bound)


@pytest.mark.parametrize('kind', ['sexp', 'matern2.5'])
def test_all_rows_in_the_set_is_the_dense_update(kind):
    """m >= n: N(x) is every training row in index order and b(x)^T r = c(x, W) R^-1 r, pathfun_ref's dense update.  Bound:
    100 times the 3e-12 the two formulations were first seen to differ by at nugget 1e-3 on values of size 3 (7e-13 and 4e-13
    on these, of size 1.5) -- numpy against itself, the factor absorbs a change of BLAS."""
    import pathfun_ref as R
    import vpathfun_ref as V
    W, y, omega, x, length, scale, nugget, _ = model(kind, 'D')
    rng = np.random.default_rng(8)
    F, P, n = 64, 4, len(W)
    Omega, b = rng.normal(size=(F, 3)), rng.uniform(0, 2 * np.pi, F)
    theta, eps = rng.normal(size=(P, F)), rng.normal(size=(P, n))
    r = R.bracket(W, y, Omega, b, theta, eps, scale, nugget, omega)
    assert np.array_equal(V.neighbours(x / length, W / length, n + 3), np.tile(np.arange(n), (len(x), 1)))
    got = V.evaluate(x, W, Omega, b, theta, r, kind, length, scale, nugget, n + 3, omega)
    want = R.evaluate(x, W, Omega, b, theta, R.weights(W, y, Omega, b, theta, eps, kind, length, scale, nugget, omega), kind, length, scale)
    print('kind %s: max |local - dense| = %.3g on values of size %.3g' % (kind, np.abs(got - want).max(), np.abs(want).max()))
    assert np.abs(got - want).max() <= 3e-10


def test_longdouble_solve_agrees_with_numpy():
    """The long-double Cholesky solve that bounds the nugget 1e-6 case of the GPU suite: the float64 solve's own error at nugget
    1e-2 is far below 1e-10."""
    import vpathfun_ref as V
    W, _, omega, x, length, _, _, m = model('matern2.5', 'D')
    xs, Ws = x / length, W / length
    NN = V.neighbours(xs, Ws, m, pad=m + 2)
    a, bl = V.coefficients(xs, Ws, NN, 'matern2.5', 1e-2, omega), V.coefficients_longdouble(xs, Ws, NN, 'matern2.5', 1e-2, omega)
    assert np.all(a[:, m:] == 0) and np.abs(a - bl.astype(float)).max() <= 1e-12
