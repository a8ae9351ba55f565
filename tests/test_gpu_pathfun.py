"""Function-valued posterior draws (dgpamd_pathfun_eval, gp.sample_functions, emulator.sample_functions; DESIGN I.12).
Needs an MI355X: -m gpu.

The reference is the numpy restatement tests/pathfun_ref.py; the tolerance of an evaluation is its forward-error bound
(pathfun_ref.tolerance), computed from the inputs of each case.  Every comparison prints the largest error / bound it met
before it asserts."""
import copy

import numpy as np
import pytest

from far_ref import check_zeros, far_inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    from dgp_amd.ops import Engine
    return Engine(0)


def npy(t):
    return t.detach().cpu().numpy()


def within(out, ref, tol, what):
    ratio = float((np.abs(np.asarray(out) - ref) / tol).max())
    print('%s: max error / bound = %.3g' % (what, ratio))
    assert ratio <= 1.0, (what, ratio)
    return ratio


def lengths(nlen, D=3):
    """One lengthscale, or one per column with a short one: arguments of the cosines in the hundreds."""
    return np.array([0.8]) if nlen == 'one' else np.concatenate(([0.6, 1.1, 0.02], np.full(D, 0.9)))[:D]


def features_for(kind, length, D, F, seed):
    from dgp_amd import pathfun
    return pathfun.features(np.random.default_rng(seed), kind, length, D, F)


# ------------------------------------------------------------------------------------------------ operator
@pytest.mark.parametrize('n', [1, 63, 64, 65, 200])
@pytest.mark.parametrize('nlen', ['one', 'D'])
@pytest.mark.parametrize('kind', ['sexp', 'matern2.5'])
def test_eval_matches_the_restatement(eng, kind, nlen, n):
    """Shared inputs (the MFMA kernel) and per-path inputs over two groups in mixed order (the lane kernel)."""
    import pathfun_ref as R
    D, scale, P = 3, 1.7, 5
    length = lengths(nlen)
    group = np.array([0, 1, 1, 0, 1])
    worst = 0.0
    for M in (1, 64, 65, 130, 2100):
        for F in (1, 64, 100, 2048):
            rng = np.random.default_rng(1000 * n + 10 * M + F)
            Omega, b = features_for(kind, length, D, F, F + n)
            W = rng.uniform(size=(2, n, D))
            theta, v = rng.normal(size=(P, F)), rng.normal(size=(P, n))
            x = rng.uniform(size=(M, D))
            out = npy(eng.pathfun_eval(kind, eng.tensor(x), eng.tensor(W[0]), eng.tensor(Omega), eng.tensor(b), eng.tensor(theta),
                                       eng.tensor(v), length, scale))
            assert out.shape == (P, M)
            ref = R.evaluate(x, W[0], Omega, b, theta, v, kind, length, scale)
            worst = max(worst, within(out, ref, R.tolerance(x, W[0], Omega, b, theta, v, kind, length, scale),
                                      'shared  %s %s n=%d M=%d F=%d' % (kind, nlen, n, M, F)))
            xs = rng.uniform(size=(P, M, D))
            out = npy(eng.pathfun_eval(kind, eng.tensor(xs), eng.tensor(W), eng.tensor(Omega), eng.tensor(b), eng.tensor(theta),
                                       eng.tensor(v), length, scale, group=group))
            for p in range(P):
                a = slice(p, p + 1)
                ref = R.evaluate(xs[p], W[group[p]], Omega, b, theta[a], v[a], kind, length, scale)
                tol = R.tolerance(xs[p], W[group[p]], Omega, b, theta[a], v[a], kind, length, scale)
                worst = max(worst, within(out[a], ref, tol, 'per-path %s %s n=%d M=%d F=%d path %d' % (kind, nlen, n, M, F, p)))
    print('worst error / bound over the case: %.3g' % worst)


@pytest.mark.parametrize('kind', ['sexp', 'matern2.5'])
def test_eval_at_64_inputs_and_without_training_rows(eng, kind):
    import pathfun_ref as R
    rng = np.random.default_rng(64)
    D, n, M, F, P, scale = 64, 130, 90, 100, 3, 1.3
    length = np.sqrt(D) * rng.uniform(0.8, 1.2, size=D)
    Omega, b = features_for(kind, length, D, F, 1)
    W, x = rng.uniform(size=(n, D)), rng.uniform(size=(M, D))
    theta, v = rng.normal(size=(P, F)), rng.normal(size=(P, n))
    t = eng.tensor
    out = npy(eng.pathfun_eval(kind, t(x), t(W), t(Omega), t(b), t(theta), t(v), length, scale))
    within(out, R.evaluate(x, W, Omega, b, theta, v, kind, length, scale),
           R.tolerance(x, W, Omega, b, theta, v, kind, length, scale), 'shared D=64 ' + kind)
    xs = rng.uniform(size=(P, M, D))
    out = npy(eng.pathfun_eval(kind, t(xs), t(W), t(Omega), t(b), t(theta), t(v), length, scale))
    for p in range(P):
        a = slice(p, p + 1)
        within(out[a], R.evaluate(xs[p], W, Omega, b, theta[a], v[a], kind, length, scale),
               R.tolerance(xs[p], W, Omega, b, theta[a], v[a], kind, length, scale), 'per-path D=64 %s path %d' % (kind, p))
    # n = 0: the prior part alone, both kernels
    D, F = 3, 2048
    length = lengths('D')
    Omega, b = features_for(kind, length, D, F, 2)
    theta, x, xs = rng.normal(size=(P, F)), rng.uniform(size=(M, D)), rng.uniform(size=(P, M, D))
    out = npy(eng.pathfun_eval(kind, t(x), None, t(Omega), t(b), t(theta), None, length, scale))
    within(out, R.evaluate(x, None, Omega, b, theta, None, kind, length, scale),
           R.tolerance(x, None, Omega, b, theta, None, kind, length, scale), 'shared n=0 ' + kind)
    out = npy(eng.pathfun_eval(kind, t(xs), None, t(Omega), t(b), t(theta), None, length, scale))
    for p in range(P):
        a = slice(p, p + 1)
        within(out[a], R.evaluate(xs[p], None, Omega, b, theta[a], None, kind, length, scale),
               R.tolerance(xs[p], None, Omega, b, theta[a], None, kind, length, scale), 'per-path n=0 %s path %d' % (kind, p))


def within_or_zero(out, ref, tol, what):
    """|out| <= 1e-300 where the reference is exactly 0 (far_ref.check_zeros), the forward-error bound everywhere else."""
    out = np.asarray(out)
    nz = check_zeros(out, ref, what)
    print('%s: %d exact zeros' % (what, (~nz).sum()))
    if nz.any():
        within(out[nz], ref[nz], tol[nz], what)


@pytest.mark.parametrize('s', [1.0, 1e4])
@pytest.mark.parametrize('kind', ['sexp', 'matern2.5'])
def test_eval_beyond_the_exponent_range(eng, kind, s):
    """n = 65 training rows and M = 70 rows of far_inputs (the first 65 rows ARE training rows: c = 1 there and 0 everywhere else),
    shared and per-path x, with random theta (the bound of every evaluation) and with theta = 0 (the correlation part alone: v[p, m]
    sqrt(scale) on the training rows, exactly 0 on the others)."""
    import pathfun_ref as R
    rng = np.random.default_rng(5)
    n, M, D, F, P, scale = 65, 70, 2, 64, 3, 1.1
    length = np.array([1e-5])
    W, x = far_inputs(n, s), far_inputs(M, s)
    xs = np.stack([x, x[::-1].copy(), np.roll(x, 3, axis=0)])
    Omega, b = features_for(kind, length, D, F, 1)
    v = rng.normal(size=(P, n))
    t = eng.tensor
    for theta in (rng.normal(size=(P, F)), np.zeros((P, F))):
        what = '%s s=%g theta %s' % (kind, s, 'random' if theta.any() else '0')
        out = npy(eng.pathfun_eval(kind, t(x), t(W), t(Omega), t(b), t(theta), t(v), length, scale))
        ref = R.evaluate(x, W, Omega, b, theta, v, kind, length, scale)
        assert theta.any() or np.count_nonzero(ref) == P * n
        within_or_zero(out, ref, R.tolerance(x, W, Omega, b, theta, v, kind, length, scale), 'shared ' + what)
        out = npy(eng.pathfun_eval(kind, t(xs), t(W), t(Omega), t(b), t(theta), t(v), length, scale))
        for p in range(P):
            a = slice(p, p + 1)
            within_or_zero(out[a], R.evaluate(xs[p], W, Omega, b, theta[a], v[a], kind, length, scale),
                           R.tolerance(xs[p], W, Omega, b, theta[a], v[a], kind, length, scale), 'per-path %s path %d' % (what, p))


@pytest.mark.parametrize('P', [1, 64, 65, 129, 300])
def test_eval_over_many_paths(eng, P):
    """More paths than one workgroup's 128 columns (shared inputs) and than one launch's 64 groups (per-path inputs)."""
    import pathfun_ref as R
    rng = np.random.default_rng(P)
    kind, D, n, M, F, scale = 'matern2.5', 5, 70, 75, 100, 0.9
    length = np.array([0.7])
    Omega, b = features_for(kind, length, D, F, 3)
    W = rng.uniform(size=(3, n, D))
    theta, v, x = rng.normal(size=(P, F)), rng.normal(size=(P, n)), rng.uniform(size=(M, D))
    t = eng.tensor
    out = npy(eng.pathfun_eval(kind, t(x), t(W[1]), t(Omega), t(b), t(theta), t(v), length, scale))
    within(out, R.evaluate(x, W[1], Omega, b, theta, v, kind, length, scale),
           R.tolerance(x, W[1], Omega, b, theta, v, kind, length, scale), 'shared P=%d' % P)
    group = rng.integers(0, 3, size=P)
    xs = rng.uniform(size=(P, M, D))
    out = npy(eng.pathfun_eval(kind, t(xs), t(W), t(Omega), t(b), t(theta), t(v), length, scale, group=group))
    for p in range(P):
        a = slice(p, p + 1)
        ratio = np.abs(out[a] - R.evaluate(xs[p], W[group[p]], Omega, b, theta[a], v[a], kind, length, scale)) / \
            R.tolerance(xs[p], W[group[p]], Omega, b, theta[a], v[a], kind, length, scale)
        assert ratio.max() <= 1.0, (p, ratio.max())


def test_eval_refuses_what_it_cannot_do(eng):
    from dgp_amd.ops import DgpAmdError
    rng = np.random.default_rng(0)
    t = eng.tensor
    x, W, Om, b = rng.uniform(size=(4, 2)), rng.uniform(size=(2, 6, 2)), rng.normal(size=(8, 2)), rng.uniform(size=8)
    th, v = rng.normal(size=(3, 8)), rng.normal(size=(3, 6))
    with pytest.raises(DgpAmdError, match='one group'):   # shared inputs and two training sets
        eng.pathfun_eval('sexp', t(x), t(W), t(Om), t(b), t(th), t(v), [1.0], 1.0, group=[0, 1, 0])
    with pytest.raises(DgpAmdError, match='out of range'):
        eng.pathfun_eval('sexp', t(np.stack([x] * 3)), t(W), t(Om), t(b), t(th), t(v), [1.0], 1.0, group=[0, 2, 0])


# ------------------------------------------------------------------------------------------------ rows are independent
@pytest.mark.parametrize('shape', ['shared', 'per-path'])
def test_rows_are_independent_bit_for_bit(eng, shape):
    """One call at 100 000 rows (above sample_paths' 8192) equals the same rows evaluated in separate slices, and a second
    evaluation equals the first."""
    import torch
    from dgp_amd.paths import MAX_POINTS
    rng = np.random.default_rng(5)
    kind, D, n, M, F, scale = 'matern2.5', 4, 200, 100000, 512, 1.1
    assert M > MAX_POINTS
    P = 70 if shape == 'shared' else 3
    length = np.array([0.5, 0.7, 0.9, 1.1])
    Omega, b = features_for(kind, length, D, F, 9)
    t = eng.tensor
    W, theta, v = t(rng.uniform(size=(n, D))), t(rng.normal(size=(P, F))), t(rng.normal(size=(P, n)))
    Om, bd = t(Omega), t(b)
    x = t(rng.uniform(size=(M, D)) if shape == 'shared' else rng.uniform(size=(P, M, D)))
    full = eng.pathfun_eval(kind, x, W, Om, bd, theta, v, length, scale)
    again = eng.pathfun_eval(kind, x, W, Om, bd, theta, v, length, scale)
    assert torch.equal(full, again)
    cuts = [0, 1, 64, 777, 33333, 33400, 99999, M]
    parts = [eng.pathfun_eval(kind, x[..., a:c, :].contiguous(), W, Om, bd, theta, v, length, scale) for a, c in zip(cuts, cuts[1:])]
    assert torch.equal(full, torch.cat(parts, 1))
    assert bool(torch.isfinite(full).all())


# ------------------------------------------------------------------------------------------------ gp
def _gp(kind, X, Y, connect=None, nugget=1e-4):
    from dgp_amd import gp, kernel
    D = X.shape[1]
    k = kernel(length=np.full(D, 0.7), name=kind, scale=1.9, nugget=nugget,
               input_dim=None if connect is None else np.setdiff1d(np.arange(D), connect), connect=connect)
    return gp(X, Y, k)


def _gp_replay(m, seed, J, F):
    """The draws gp.sample_functions takes from a global generator seeded with `seed`, in its documented order."""
    from dgp_amd import pathfun
    k = m.kernel
    W = k._X()
    np.random.seed(seed)
    Omega, b = pathfun.features(np.random, k.name, k.length, W.shape[1], F)
    theta = np.random.standard_normal((J, F))
    eps = np.random.standard_normal((J, len(W)))
    return W, Omega, b, theta, eps


@pytest.mark.parametrize('case', ['matern2.5-replicates-connect', 'sexp-plain'])
def test_gp_sample_functions_replays_numpy(eng, case):
    import pathfun_ref as R
    kind = case.split('-')[0]
    rng = np.random.default_rng(11)
    X = rng.uniform(size=(60, 3))
    connect = None
    if 'replicates' in case:
        X, connect = np.concatenate((X, X[:15])), np.array([2])
    Y = (np.sin(3 * X[:, 0]) + X[:, 1] * X[:, 2] + 0.05 * rng.normal(size=len(X)))[:, None]
    m = _gp(kind, X, Y, connect=connect)
    k = m.kernel
    J, F = 7, 300
    np.random.seed(21)
    paths = m.sample_functions(sample_size=J, n_features=F)
    state = np.random.get_state()
    W, Omega, b, theta, eps = _gp_replay(m, 21, J, F)
    assert all(np.array_equal(a, c) for a, c in zip(state[1:], np.random.get_state()[1:]))   # nothing else was drawn
    cols = np.arange(3) if connect is None else np.concatenate((np.setdiff1d(np.arange(3), connect), connect))
    omega = None if k.rep is None else k.W_diag
    assert (omega is not None) == ('replicates' in case)
    y, s, eta = np.asarray(k.output, float).reshape(-1), k.scale[0], k.nugget[0]
    v = R.weights(W, y, Omega, b, theta, eps, kind, k.length, s, eta, omega)
    x1, x2 = rng.uniform(size=(35, 3)), rng.uniform(size=(50, 3))
    o1, o2 = paths(x1), paths(x2)
    assert o1.shape == (35, J)
    for x, o in ((x1, o1), (x2, o2)):
        within(o.T, R.evaluate(x[:, cols], W, Omega, b, theta, v, kind, k.length, s),
               R.tolerance(x[:, cols], W, Omega, b, theta, v, kind, k.length, s), 'gp %s' % case)
    # a path is a function: the union of two sets of rows gives the two evaluations, and a second call the same values
    both = paths(np.concatenate((x1, x2)))
    assert np.array_equal(both, np.concatenate((o1, o2))) and np.array_equal(paths(x1), o1)
    # at the training rows: f(W) / sqrt(s) - y / sqrt(s) = -sqrt(eta omega) eps - eta omega R^-1 r
    Xtr = np.empty((len(W), 3))
    Xtr[:, cols] = W
    om = np.ones(len(W)) if omega is None else omega
    want = -np.sqrt(eta * om) * eps - eta * om * v
    got = (paths(Xtr).T - y) / np.sqrt(s)
    within(got, want, R.tolerance(W, W, Omega, b, theta, v, kind, k.length, s) / np.sqrt(s), 'gp %s at the training rows' % case)
    # noise=True: one standard_normal((J, M)) block, scaled by sqrt(s eta), on top of the same function values
    np.random.seed(5)
    noisy = paths(x1, noise=True)
    np.random.seed(5)
    assert np.allclose(noisy, o1 + np.sqrt(s * eta) * np.random.standard_normal((J, 35)).T, rtol=0, atol=1e-14)


def test_gp_paths_have_the_posterior_moments(eng):
    """4000 paths of a gp with n = 50 at M = 20 rows, F = 4096, noise=True: the sample mean within 5 standard errors of
    dgpamd_joint_cov's mean, the sample covariance within 6 of its standard errors sqrt((C_ii C_jj + C_ij^2) / P) of
    C = the restatement's implied covariance + s eta I."""
    import pathfun_ref as R
    from dgp_amd import paths as dpaths
    X, Y, x, kind, length, s, eta, F, P = R.dist_case()
    M = len(x)
    m = _gp(kind, X, Y, nugget=eta)
    k = m.kernel
    assert np.array_equal(k.length, length) and k.scale[0] == s and k.nugget[0] == eta and np.array_equal(k._X(), X)
    np.random.seed(R.SEED_DIST)
    draws = m.sample_functions(sample_size=P, n_features=F)(x, noise=True)
    assert draws.shape == (M, P)
    W, Omega, b, _, _ = _gp_replay(m, R.SEED_DIST, 1, F)
    y = np.asarray(k.output, float).reshape(-1)
    _, C, _ = R.moments(x, W, y, Omega, b, kind, length, s, eta)
    C = C + s * eta * np.eye(M)
    Linv = dpaths.factor_inverse(eng, k.name, eng.tensor(W), None, None, k.length, eta, 'test')
    A, mean = eng.joint_cov(k.name, eng.tensor(x), eng.tensor(W), Linv, eng.tensor(y.reshape(1, -1)), k.length, s, eta)
    zm, zc = R.dist_z(draws, npy(mean[0])[:, 0], npy(A[0])[:M, :M], C)
    print('mean: max z = %.3g (5); covariance: max z = %.3g (6)' % (zm, zc))
    assert zm <= 5.0 and zc <= 6.0


# ------------------------------------------------------------------------------------------------ emulator
def _model(which, kind='matern2.5'):
    from dgp_amd import dgp, kernel, combine, Hetero, Categorical
    rng = np.random.default_rng(6)
    K = lambda **kw: kernel(length=np.array([1.0]), name=kind, nugget=1e-4, **kw)
    if which == 'two-connect':
        X = rng.uniform(size=(60, 2))
        Y = np.sin(5 * X[:, :1]) * np.cos(3 * X[:, 1:]) + 0.02 * rng.normal(size=(60, 1))
        layers = combine([K(), K()], [K(scale_est=True, connect=np.arange(2))])
    elif which == 'three':
        X = rng.uniform(size=(50, 2))
        Y = np.sin(5 * X[:, :1]) + X[:, 1:] ** 2 + 0.02 * rng.normal(size=(50, 1))
        layers = combine([K(), K()], [K(), K()], [K(scale_est=True)])
    elif which == 'hetero':
        x = np.sort(rng.uniform(size=60))
        X = x[:, None]
        Y = (np.sin(6 * x) + (0.05 + 0.5 * x ** 2) * rng.normal(size=60))[:, None]
        layers = combine([kernel(length=np.array([0.5]), name='sexp', scale_est=True),
                          kernel(length=np.array([0.5]), name='sexp', scale_est=True)], [Hetero()])
    else:
        X = rng.uniform(size=(50, 2))
        Y = (X[:, [0]] + 0.3 * np.sin(6 * X[:, [1]]) > 0.55).astype(int)
        layers = combine([K(), K()], [K(scale_est=True)], [Categorical(num_classes=2)])
    model = dgp(X, Y, layers, seed=4)
    model.train(N=3, ess_burn=3, disable=True)
    return X, model


@pytest.mark.parametrize('which', ['two-connect', 'three', 'hetero', 'categorical'])
def test_emulator_sample_functions_replays_the_layer_walk(eng, which):
    """Node by node: the restatement, given the generator's draws in the documented order, at the device's own outputs of
    the layer below, so the tolerance stays the bound of one node's evaluation."""
    import pathfun_ref as R
    from dgp_amd import emulator, pathfun
    X, model = _model(which)
    emu = emulator(model.estimate(), N=2, seed=5)
    S, J, F, M = 2, 3, 200, 40
    x = np.random.default_rng(8).uniform(size=(M, X.shape[1]))
    rng = copy.deepcopy(emu._sample_rng)
    pf = emu.sample_functions(sample_size=J, n_features=F)
    assert isinstance(pf, pathfun.PathFunctions)
    out = pf(x, full_layer=True)
    # the container of sample_paths
    ref_out = emu.sample_paths(x, sample_size=J, full_layer=True)
    assert len(out) == len(ref_out)
    for a, c in zip(out, ref_out):
        assert len(a) == len(c) and all(u.shape == w.shape == (M, S * J) for u, w in zip(a, c))
    last = pf(x)
    assert len(last) == len(out[-1])
    for l, layer in enumerate(emu.all_layer):
        for k, nd in enumerate(layer):
            if nd.type != 'gp':
                continue
            D = nd._X().shape[1] if l == 0 else len(nd.input_dim) + (0 if nd.connect is None else len(nd.connect))
            Omega, b = pathfun.features(rng, nd.name, nd.length, D, F)
            theta, eps = rng.standard_normal((S, J, F)), rng.standard_normal((S, J, len(nd.output)))
            gl = None if nd.connect is None else x[:, nd.connect]
            omega = None if nd.rep is None else nd.W_diag
            for s in range(S):
                y = emu.latents[s][l][:, k] if l < emu.n_layer - 1 else np.asarray(nd.output, float).reshape(-1)
                if l == 0:
                    W = nd._X()
                else:
                    W = emu.latents[s][l - 1][:, nd.input_dim]
                    if nd.connect is not None:
                        W = np.concatenate((W, nd.global_input), 1)
                v = R.weights(W, y, Omega, b, theta[s], eps[s], nd.name, nd.length, nd.scale[0], nd.nugget[0], omega)
                for j in range(J):
                    p, a = s * J + j, slice(j, j + 1)
                    xin = x[:, nd.input_dim] if l == 0 else np.stack([out[l - 1][kk][:, p] for kk in nd.input_dim], 1)
                    if gl is not None:
                        xin = np.concatenate((xin, gl), 1)
                    ref = R.evaluate(xin, W, Omega, b, theta[s][a], v[a], nd.name, nd.length, nd.scale[0])
                    tol = R.tolerance(xin, W, Omega, b, theta[s][a], v[a], nd.name, nd.length, nd.scale[0])
                    within(out[l][k][:, p][None], ref, tol, '%s layer %d node %d path %d' % (which, l + 1, k + 1, p))
    # GP layers are functions: a second evaluation gives the same values; likelihood layers are sampled afresh
    again = pf(x, full_layer=True)
    for l, layer in enumerate(emu.all_layer):
        for k, nd in enumerate(layer):
            if nd.type == 'gp':
                assert np.array_equal(again[l][k], out[l][k])
    top = emu.all_layer[-1][0]
    if which == 'hetero':
        assert top.type == 'likelihood' and np.all(np.isfinite(out[-1][0]))
    if which == 'categorical':
        from scipy.special import expit
        np.testing.assert_allclose(out[-1][0], expit(out[-2][0]), rtol=1e-14, atol=0)
    # noise=True adds one N(0, scale nugget) block per GP node in walk order, from the emulator's generator
    if which == 'two-connect':
        state = copy.deepcopy(emu._sample_rng)
        noisy = pf(x, full_layer=True, noise=True)
        for k, nd in enumerate(emu.all_layer[0]):
            z = state.standard_normal((S * J, M))
            np.testing.assert_allclose(noisy[0][k], out[0][k] + np.sqrt(nd.scale[0] * nd.nugget[0]) * z.T, rtol=0, atol=1e-13)


def test_refusals(eng):
    from dgp_amd import emulator, gp, kernel
    rng = np.random.default_rng(2)
    X = rng.uniform(size=(40, 2))
    Y = np.sin(4 * X[:, :1])
    vg = gp(X, Y, kernel(length=np.array([0.5]), name='sexp'), vecchia=True, m=10)
    with pytest.raises(NotImplementedError, match='sample_paths needs a dense GP'):
        vg.sample_functions()
    _, model = _model('two-connect', 'sexp')
    emu = emulator(model.estimate(), N=2, seed=1)
    emu.to_vecchia()
    with pytest.raises(NotImplementedError, match='sample_paths needs a dense emulator'):
        emu.sample_functions()
    emu.remove_vecchia()
    emu.shard = True
    with pytest.raises(NotImplementedError, match='sharded over ranks'):
        emu.sample_functions()
    emu.shard = False
    pf = emu.sample_functions(sample_size=2, n_features=16)
    with pytest.raises(Exception, match='2d-array'):
        pf(X[0])
    with pytest.raises(ValueError, match='no rows'):
        pf(X[:0])


def test_indefinite_training_matrix_raises(eng):
    from dgp_amd import kernel, emulator
    rng = np.random.default_rng(9)
    n = 40
    X = rng.uniform(size=(n, 2))
    X[17] = X[4]
    y = np.sin(4 * X[:, 0]) + X[:, 1]
    y[17] = y[4]
    nd = kernel(length=np.array([0.6, 0.9]), name='matern2.5', nugget=-1e-3, scale=1.7)
    nd.input, nd.output, nd.global_input, nd.engine = X, y[:, None], None, eng
    nd.input_dim, nd.D = np.arange(2), 2
    nd.compute_stats()
    emu = emulator([[nd]], N=1)
    with pytest.raises(np.linalg.LinAlgError, match='layer 1, node 1'):
        emu.sample_functions(sample_size=3, n_features=32)


# ------------------------------------------------------------------------------------------------ row blocks, the builder
@pytest.mark.parametrize('which', ['two-connect', 'three'])
def test_emulator_row_blocks_change_no_bit_and_draw_noise_per_block(eng, which, monkeypatch):
    """Blocks of 7 rows at M = 40: every GP layer of paths(x) bit for bit the unblocked call's; with noise=True every GP node
    in walk order, block by block, takes one standard_normal((N * J, rows of the block)) from the emulator's generator: its
    result is its paths at the (noisy) inputs it was given plus sqrt(scale nugget) times those normals."""
    from dgp_amd import emulator, pathfun
    X, model = _model(which)
    emu = emulator(model.estimate(), N=2, seed=5)
    S, J, F, M = 2, 3, 200, 40
    x = np.random.default_rng(8).uniform(size=(M, X.shape[1]))
    pf = emu.sample_functions(sample_size=J, n_features=F)
    whole = pf(x, full_layer=True)
    monkeypatch.setattr(pathfun, '_rows_per_call', lambda e, P, width: 7)
    blocked = pf(x, full_layer=True)
    assert len(whole) == len(blocked) == emu.n_layer
    for a, c in zip(whole, blocked):
        assert len(a) == len(c) and all(np.array_equal(u, w) and u.shape == (M, S * J) for u, w in zip(a, c))
    state = copy.deepcopy(emu._sample_rng)
    noisy = pf(x, full_layer=True, noise=True)
    z = [[np.empty((M, S * J)) for _ in layer] for layer in emu.all_layer]
    for m0 in range(0, M, 7):
        for l, layer in enumerate(emu.all_layer):
            for k in range(len(layer)):
                z[l][k][m0:m0 + 7] = state.standard_normal((S * J, min(7, M - m0))).T
    assert emu._sample_rng.bit_generator.state == state.bit_generator.state   # nothing else was drawn
    e = pf.engine
    for l, layer in enumerate(emu.all_layer):
        for k, nd in enumerate(layer):
            if l == 0:
                values = whole[0][k]
            else:   # the node's paths at the noisy outputs of the layer below: rows are independent, so these are the walk's bits
                xin = np.stack([np.stack([noisy[l - 1][kk][:, p] for kk in nd.input_dim], 1) for p in range(S * J)])
                if nd.connect is not None:
                    xin = np.concatenate((xin, np.broadcast_to(x[:, nd.connect], (S * J, M, len(nd.connect)))), 2)
                values = npy(pf.nodes[l, k](e, e.tensor(xin))).T
            dev = np.abs(noisy[l][k] - (values + np.sqrt(nd.scale[0] * nd.nugget[0]) * z[l][k])).max()
            print('%s layer %d node %d: max |noisy - (values + sd z)| = %.3g (1e-13)' % (which, l + 1, k + 1, dev))
            assert dev <= 1e-13


def _gp_case(case, rng, n=60, rep=15):
    """test_gp_sample_functions_replays_numpy's models: n distinct rows, with 'replicates' the first `rep` twice and a
    `connect` column."""
    X = rng.uniform(size=(n, 3))
    connect = None
    if 'replicates' in case:
        X, connect = np.concatenate((X, X[:rep])), np.array([2])
    Y = (np.sin(3 * X[:, 0]) + X[:, 1] * X[:, 2] + 0.05 * rng.normal(size=len(X)))[:, None]
    return _gp(case.split('-')[0], X, Y, connect=connect)


@pytest.mark.parametrize('case', ['matern2.5-replicates-connect', 'sexp-plain'])
def test_gp_row_blocks_change_no_bit_and_draw_noise_once(eng, case, monkeypatch):
    """Blocks of 7 rows at M = 35: paths(x) and value_and_grad(x) bit for bit the unblocked calls'; noise=True still takes one
    np.random.standard_normal((J, 35)) for all rows."""
    from dgp_amd import pathfun
    rng = np.random.default_rng(11)
    m = _gp_case(case, rng)
    J = 3
    np.random.seed(21)
    paths = m.sample_functions(sample_size=J, n_features=200)
    x = rng.uniform(size=(35, 3))
    whole, (vals, grad) = paths(x), paths.value_and_grad(x)
    monkeypatch.setattr(pathfun, '_rows_per_call', lambda e, P, width: 7)
    assert np.array_equal(paths(x), whole)
    v2, g2 = paths.value_and_grad(x)
    assert np.array_equal(v2, vals) and np.array_equal(g2, grad) and np.array_equal(vals, whole) and grad.shape == (35, 3, J)
    s, eta = m.kernel.scale[0], m.kernel.nugget[0]
    np.random.seed(5)
    noisy = paths(x, noise=True)
    np.random.seed(5)
    assert np.allclose(noisy, whole + np.sqrt(s * eta) * np.random.standard_normal((J, 35)).T, rtol=0, atol=1e-14)


def test_builders_take_the_dense_drawer_s_training_side(eng):
    """A gp model's (Wall, L^-1), n = 30, D = 3, matern2.5 with replicates, and two rows of right-hand sides -- what
    paths.Dense.draw_shared and draw_per_path are given -- through build_shared (rep = J) and build_per_group (PerGroup views,
    group = repeat(arange(2), J)) with the same draws: each against the restatement at 35 rows.  The second group of
    build_per_group has training inputs of its own (the model's, shifted) with their own L^-1."""
    import pathfun_ref as R
    from dgp_amd import pathfun
    from dgp_amd import paths as dpaths
    rng = np.random.default_rng(12)
    m = _gp_case('matern2.5-replicates-connect', rng, n=30, rep=8)
    k = m.kernel
    e = k.engine
    train = m._joint_train()
    W, (n, D) = k._X(), k._X().shape
    omega = e.tensor(k.W_diag)
    assert (n, D) == (30, 3) and k.rep is not None and np.array_equal(npy(train[0]), W)
    S, J, F, M = 2, 3, 200, 35
    y = np.asarray(k.output, float).reshape(-1)
    Y = np.stack((y, y + 0.5))
    hyper = dpaths.hyper(k)
    kind, length, s, eta = hyper
    Omega, b, theta, eps = pathfun.draw_node(np.random.default_rng(3), kind, length, D, F, S, J, n)
    draws = [e.tensor(a) for a in (Omega, b, theta, eps)]
    W2 = W + 0.05 * rng.uniform(size=W.shape)
    W2d = e.tensor(W2)
    Linv2 = dpaths.factor_inverse(e, kind, W2d[:, :2].contiguous(), W2d[:, 2:].contiguous(), omega, length, eta, 'test')
    trains = [train, (W2d, Linv2)]
    Yd = e.tensor(Y)
    shared = pathfun.NodePaths.build_shared(e, hyper, train, Yd, omega, draws, J)
    grouped = pathfun.NodePaths.build_per_group(e, hyper, dpaths.PerGroup(lambda g: trains[g]), dpaths.PerGroup(lambda g: Yd[g]),
                                                omega, draws, np.repeat(np.arange(S), J))
    assert shared.W.shape == (n, D) and shared.group is None and shared.W.data_ptr() != train[0].data_ptr()
    assert grouped.W.shape == (S, n, D) and np.array_equal(grouped.group, np.repeat(np.arange(S), J))
    x = rng.uniform(size=(M, D))
    v = R.weights(W, np.repeat(Y, J, 0), Omega, b, theta, eps, kind, length, s, eta, k.W_diag)
    within(npy(shared(e, e.tensor(x))), R.evaluate(x, W, Omega, b, theta, v, kind, length, s),
           R.tolerance(x, W, Omega, b, theta, v, kind, length, s), 'build_shared')
    out = npy(grouped(e, e.tensor(np.broadcast_to(x, (S * J, M, D)).copy())))
    for g, Wg in enumerate((W, W2)):
        a = slice(g * J, (g + 1) * J)
        vg = R.weights(Wg, Y[g], Omega, b, theta[a], eps[a], kind, length, s, eta, k.W_diag)
        assert g == 0 or np.abs(vg - v[a]).max() > 1e-3 * np.abs(vg).max()   # (the second training set matters)
        within(out[a], R.evaluate(x, Wg, Omega, b, theta[a], vg, kind, length, s),
               R.tolerance(x, Wg, Omega, b, theta[a], vg, kind, length, s), 'build_per_group, group %d' % g)
