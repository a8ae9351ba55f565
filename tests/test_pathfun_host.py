"""Host-side pieces of the function-valued posterior draws (no GPU; DESIGN I.12): the public signatures, the random-Fourier-
feature sampler of dgp_amd.pathfun against the oracle's correlations, and the moments of the numpy restatement
(tests/pathfun_ref.py) that the GPU tests compare the device against."""
import inspect

import numpy as np
import pytest

F_BIG = 65536


def feature_bound(F):
    """6 standard deviations of one entry of Phi Phi^T, the mean of F terms 2 cos(a) cos(b) = cos(a - b) + cos(a + b): a + b
    has a uniform phase, so a term has mean k = E cos(a - b) and variance E cos^2(a - b) + 1/2 - k^2 <= 1.5."""
    return 6.0 * np.sqrt(1.5 / F)


def test_sample_functions_signatures():
    from dgp_amd import emulator, gp
    p = inspect.signature(emulator.sample_functions).parameters
    assert list(p) == ['self', 'sample_size', 'n_features']
    assert p['sample_size'].default == 50 and p['n_features'].default == 2048
    p = inspect.signature(gp.sample_functions).parameters
    assert list(p) == ['self', 'sample_size', 'n_features']
    assert p['sample_size'].default == 50 and p['n_features'].default == 2048
    from dgp_amd import pathfun
    p = inspect.signature(pathfun.PathFunctions.__call__).parameters
    assert list(p) == ['self', 'x', 'full_layer', 'noise'] and p['full_layer'].default is False and p['noise'].default is False
    p = inspect.signature(pathfun.GpPaths.__call__).parameters
    assert list(p) == ['self', 'x', 'noise'] and p['noise'].default is False


def test_eval_entry_is_declared_without_a_workspace():
    """dgpamd_pathfun_eval stores neither the features nor the correlations: there is no workspace formula to test."""
    from dgp_amd import _lib
    assert 'dgpamd_pathfun_eval' in _lib.SIGNATURES and 'dgpamd_pathfun_workspace' not in _lib.SIGNATURES
    assert len(_lib.SIGNATURES['dgpamd_pathfun_eval'][1]) == 21


@pytest.mark.parametrize('nlen', ['one', 'D'])
@pytest.mark.parametrize('kind', ['sexp', 'matern2.5'])
def test_feature_sampler_reproduces_the_correlation(kind, nlen):
    """max |Phi(W) Phi(x)^T - c(W, x)| <= 6 sqrt(1.5 / F) at F = 65536, with the sampler's own draw order."""
    from dgp_amd import pathfun
    from oracle import dgp_oracle as O
    import pathfun_ref as R
    D = 3
    length = np.array([0.8]) if nlen == 'one' else np.array([0.6, 1.1, 0.9])
    rng = np.random.default_rng(11)
    W, x = rng.uniform(size=(40, D)), rng.uniform(size=(50, D))
    Omega, b = pathfun.features(np.random.default_rng(2024), kind, length, D, F_BIG)
    assert Omega.shape == (F_BIG, D) and b.shape == (F_BIG,) and b.min() >= 0.0 and b.max() < 2 * np.pi
    err = np.abs(R.phi(W, Omega, b) @ R.phi(x, Omega, b).T - O.cross_corr(W, x, length, kind)).max()
    print('kind %s, lengths %s: max |Phi Phi^T - K| = %.4g (bound %.4g)' % (kind, nlen, err, feature_bound(F_BIG)))
    assert err <= feature_bound(F_BIG)


def test_feature_sampler_draw_order():
    """standard_normal((F, D)), chisquare(5, (F, D)) for matern2.5 only, uniform(0, 2 pi, F) -- from a Generator or from the
    numpy.random module (gp.sample_functions)."""
    from dgp_amd import pathfun
    F, D, g = 7, 2, np.array([0.5, 2.0])
    for kind in ('sexp', 'matern2.5'):
        r = np.random.default_rng(5)
        z = r.standard_normal((F, D))
        want = np.sqrt(2.0) * z / g if kind == 'sexp' else z / np.sqrt(r.chisquare(5, (F, D)) / 5.0) / g
        wb = r.uniform(0.0, 2.0 * np.pi, F)
        Omega, b = pathfun.features(np.random.default_rng(5), kind, g, D, F)
        assert np.array_equal(Omega, want) and np.array_equal(b, wb)
        np.random.seed(9)
        O1, b1 = pathfun.features(np.random, kind, g, D, F)
        np.random.seed(9)
        z = np.random.standard_normal((F, D))
        want = np.sqrt(2.0) * z / g if kind == 'sexp' else z / np.sqrt(np.random.chisquare(5, (F, D)) / 5.0) / g
        assert np.array_equal(O1, want) and np.array_equal(b1, np.random.uniform(0.0, 2.0 * np.pi, F))
    Omega, _ = pathfun.features(np.random.default_rng(5), 'sexp', np.array([0.5]), 3, F)   # one lengthscale for every column
    assert np.array_equal(Omega, np.sqrt(2.0) * np.random.default_rng(5).standard_normal((F, 3)) / 0.5)


@pytest.mark.parametrize('F', [1, 64, 4096])
@pytest.mark.parametrize('kind', ['sexp', 'matern2.5'])
def test_restatement_moments(kind, F):
    """The restatement is affine in (theta, eps): its mean is its value at (0, 0), c(x, W) R^-1 y to rounding for every F;
    its linear part gives the covariance s (A A^T + eta B diag(omega) B^T), which lies within
    (1 + |B_i|_1)(1 + |B_j|_1) 6 sqrt(1.5 / F) s of the exact posterior covariance: [I, -B] applied on both sides to the error
    of the feature estimate of the joint kernel over (x, W)."""
    from dgp_amd import pathfun
    from oracle import dgp_oracle as O
    import pathfun_ref as R
    rng = np.random.default_rng(F + 3)
    D, n, M, scale, nugget = 3, 30, 12, 1.7, 1e-2
    length = np.array([0.6, 1.1, 0.9])
    W, x, y = rng.uniform(size=(n, D)), rng.uniform(size=(M, D)), rng.normal(size=n)
    omega = 1.0 / rng.integers(1, 4, size=n)
    Omega, b = pathfun.features(np.random.default_rng(77), kind, length, D, F)
    f = lambda th, ep: R.evaluate(x, W, Omega, b, th, R.weights(W, y, Omega, b, th, ep, kind, length, scale, nugget, omega),
                                  kind, length, scale)
    mean, cov, B = R.moments(x, W, y, Omega, b, kind, length, scale, nugget, omega)
    want = O.cross_corr(W, x, length, kind).T @ np.linalg.solve(R.train_corr(W, kind, length, nugget, omega), y)
    th, ep = rng.normal(size=(5, F)), rng.normal(size=(5, n))
    mid = 0.5 * (f(th, ep) + f(-th, -ep))
    tol = 1e-9 * (1.0 + np.abs(want).max())
    assert np.abs(mid - want).max() <= tol and np.abs(mean - want).max() <= tol
    assert np.abs(f(np.zeros((1, F)), np.zeros((1, n)))[0] - want).max() <= tol
    # the linear part, column by column
    f0 = f(np.zeros((1, F)), np.zeros((1, n)))[0]
    Jt = (f(np.eye(F), np.zeros((F, n))) - f0).T if F <= 64 else None
    Je = (f(np.zeros((n, F)), np.eye(n)) - f0).T
    if Jt is not None:
        assert np.abs(Jt @ Jt.T + Je @ Je.T - cov).max() <= 1e-8 * scale
    exact = R.exact_cov(x, W, kind, length, scale, nugget, omega)
    l1 = 1.0 + np.abs(B).sum(1)
    bound = scale * np.outer(l1, l1) * feature_bound(F)
    print('kind %s, F %d: max |cov - exact| / bound = %.3g' % (kind, F, (np.abs(cov - exact) / bound).max()))
    assert np.all(np.abs(cov - exact) <= bound)


def test_restatement_alone_passes_the_distributional_check():
    """The seed of the GPU suite's distributional check (pathfun_ref.SEED_DIST) is one with which the restatement, fed the
    draws gp.sample_functions documents (features, theta, eps, then the noise block of the evaluation), passes both
    conditions by itself: sample mean within 5 standard errors of the exact posterior mean, sample covariance within 6 of
    the implied covariance + s eta I."""
    from dgp_amd import pathfun
    import pathfun_ref as R
    X, Y, x, kind, length, s, eta, F, P = R.dist_case()
    W, y = X, Y[:, 0]
    np.random.seed(R.SEED_DIST)
    Omega, b = pathfun.features(np.random, kind, length, 2, F)
    theta, eps = np.random.standard_normal((P, F)), np.random.standard_normal((P, len(W)))
    v = R.weights(W, y, Omega, b, theta, eps, kind, length, s, eta)
    draws = R.evaluate(x, W, Omega, b, theta, v, kind, length, s).T + np.sqrt(s * eta) * np.random.standard_normal((P, len(x))).T
    mean, C, _ = R.moments(x, W, y, Omega, b, kind, length, s, eta)
    noise = s * eta * np.eye(len(x))
    zm, zc = R.dist_z(draws, mean, R.exact_cov(x, W, kind, length, s, eta) + noise, C + noise)
    print('restatement, seed %d: mean max z = %.3g (5); covariance max z = %.3g (6)' % (R.SEED_DIST, zm, zc))
    assert zm <= 5.0 and zc <= 6.0


@pytest.mark.parametrize('nlen', ['one', 'D'])
@pytest.mark.parametrize('kind', ['sexp', 'matern2.5'])
def test_draw_node_consumes_the_generator_in_the_documented_order(kind, nlen):
    """features (normals (F, D), chi^2_5 for matern2.5, phases), then standard_normal((S, J, F)), then standard_normal((S, J,
    n)), and nothing else; with S = 1 on numpy's global generator, the order gp.sample_functions documents."""
    from dgp_amd import pathfun
    S, J, F, n, D = 2, 3, 5, 4, 3
    length = np.array([0.8]) if nlen == 'one' else np.array([0.6, 1.1, 0.9])
    g = np.broadcast_to(length, (D,))
    rng, r = np.random.default_rng(31), np.random.default_rng(31)
    Omega, b, theta, eps = pathfun.draw_node(rng, kind, length, D, F, S, J, n)
    z = r.standard_normal((F, D))
    want = np.sqrt(2.0) * z / g if kind == 'sexp' else z / np.sqrt(r.chisquare(5, (F, D)) / 5.0) / g
    assert np.array_equal(Omega, want) and np.array_equal(b, r.uniform(0.0, 2.0 * np.pi, F))
    assert theta.shape == (S * J, F) and np.array_equal(theta, r.standard_normal((S, J, F)).reshape(S * J, F))
    assert eps.shape == (S * J, n) and np.array_equal(eps, r.standard_normal((S, J, n)).reshape(S * J, n))
    assert rng.bit_generator.state == r.bit_generator.state
    # an iterator: asked for Omega and b alone, it has drawn the features alone
    it = pathfun.draw_node(rng, kind, length, D, F, S, J, n)
    next(it), next(it)
    pathfun.features(r, kind, length, D, F)
    assert rng.bit_generator.state == r.bit_generator.state
    np.random.seed(9)
    got = list(pathfun.draw_node(np.random, kind, length, D, F, 1, J, n))
    np.random.seed(9)
    z = np.random.standard_normal((F, D))
    want = np.sqrt(2.0) * z / g if kind == 'sexp' else z / np.sqrt(np.random.chisquare(5, (F, D)) / 5.0) / g
    wb = np.random.uniform(0.0, 2.0 * np.pi, F)
    wt, we = np.random.standard_normal((J, F)), np.random.standard_normal((J, n))
    assert all(np.array_equal(a, c) for a, c in zip(got, (want, wb, wt, we)))
    state = np.random.get_state()
    np.random.seed(9)
    list(pathfun.draw_node(np.random, kind, length, D, F, 1, J, n))
    assert all(np.array_equal(a, c) for a, c in zip(state[1:], np.random.get_state()[1:]))


@pytest.mark.parametrize('step', [1, 7, 40, 1000])
def test_row_blocks_tile_the_rows_once_and_in_order(step, monkeypatch):
    from dgp_amd import pathfun
    monkeypatch.setattr(pathfun, '_rows_per_call', lambda e, P, width: step)
    M = 40
    x = np.arange(2 * M, dtype=float).reshape(M, 2)[:, ::-1]   # (not contiguous)
    blocks = list(pathfun._row_blocks(None, x, 6, 10))
    assert [m0 for m0, _ in blocks] == list(range(0, M, step))
    assert all(xb.flags['C_CONTIGUOUS'] and 1 <= len(xb) <= step for _, xb in blocks)
    assert np.array_equal(np.concatenate([xb for _, xb in blocks]), x)
    with pytest.raises(ValueError, match='sample_functions: x has no rows'):
        list(pathfun._row_blocks(None, x[:0], 6, 10))

