"""emulator.sample_functions_vecchia and gp.sample_functions_vecchia (DESIGN I.14) on small models (n <= 80, F = 64): the
objects against the numpy replay of tests/vpathfun_ref.py built from the generator's draws in the documented order, node by
node at the device's own outputs of the layer below (as tests/test_gpu_pathfun.py carries a bound through a layer).
Bound of one node per (path, row): the operator's sqrt(s) (1e-8 sum_j |b_j r_j| + 1e-10), plus I.12's evaluation bound for the
prior part at x, plus the same bound for the prior part inside the device's own residuals r (at W), carried through |b|.
Needs an MI355X: -m gpu."""
import copy
import warnings

import numpy as np
import pytest

import pathfun_ref as R
import vpathfun_ref as V
from test_gpu_pathfun import _gp, _gp_replay, _model, within

pytestmark = pytest.mark.gpu
F = 64


@pytest.fixture(scope='module')
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    from dgp_amd.ops import default_engine
    return default_engine(0)


def replay(x, W, Omega, b, theta, r, kind, length, s, eta, m, omega):
    """(f (P, M), bound (P, M)) of the locally conditioned paths at x (M, D) shared by the P paths."""
    xs, Ws = x / length, W / length
    NN = V.neighbours(xs, Ws, m)
    B = V.coefficients(xs, Ws, NN, kind, eta, omega)
    upd, mag = V.update(B, NN, r)
    tol_r = R.tolerance(W, None, Omega, b, theta, None, kind, length, 1.0) + 4 * R.EPS * np.abs(r)
    tol = np.sqrt(s) * (1e-8 * mag + 1e-10 + V.update(np.abs(B), NN, tol_r)[0]) + R.tolerance(x, None, Omega, b, theta, None, kind, length, s)
    return np.sqrt(s) * (theta @ R.phi(x, Omega, b).T + upd), tol


def walk_ref(emu, x, rng, J, m, forced=None):
    """The numpy walk of an emulator of GP nodes with the draws of `rng` in sample_functions' order: per layer (K, M, P)
    values and bounds.  m None: pathfun_ref's dense paths; else the local conditioning on m rows.  forced: the device's
    container -- every node is then evaluated at the device's own outputs of the layer below."""
    from dgp_amd import pathfun
    S, M = emu.N, len(x)
    outs, tols = [], []
    for l, layer in enumerate(emu.all_layer):
        cur, tol = np.zeros((len(layer), M, S * J)), np.zeros((len(layer), M, S * J))
        for k, nd in enumerate(layer):
            D = nd._X().shape[1] if l == 0 else len(nd.input_dim) + (0 if nd.connect is None else len(nd.connect))
            Omega, b = pathfun.features(rng, nd.name, nd.length, D, F)
            theta, eps = rng.standard_normal((S, J, F)), rng.standard_normal((S, J, len(nd.output)))
            gl = None if nd.connect is None else x[:, nd.connect]
            omega = None if nd.rep is None else nd.W_diag
            hyp = (nd.name, nd.length, nd.scale[0])
            for s in range(S):
                y = emu.latents[s][l][:, k] if l < emu.n_layer - 1 else np.asarray(nd.output, float).reshape(-1)
                W = nd._X() if l == 0 else emu.latents[s][l - 1][:, nd.input_dim]
                if l > 0 and nd.connect is not None:
                    W = np.concatenate((W, nd.global_input), 1)
                r = R.bracket(W, y, Omega, b, theta[s], eps[s], nd.scale[0], nd.nugget[0], omega)
                v = np.linalg.solve(R.train_corr(W, nd.name, nd.length, nd.nugget[0], omega), r.T).T if m is None else None
                for j in range(J):
                    p, a = s * J + j, slice(j, j + 1)
                    below = None if l == 0 else (outs[l - 1] if forced is None else forced[l - 1])
                    xin = x[:, nd.input_dim] if l == 0 else np.stack([below[kk][:, p] for kk in nd.input_dim], 1)
                    if gl is not None:
                        xin = np.concatenate((xin, gl), 1)
                    if m is None:
                        cur[k][:, p] = R.evaluate(xin, W, Omega, b, theta[s][a], v[a], *hyp)[0]
                        tol[k][:, p] = R.tolerance(xin, W, Omega, b, theta[s][a], v[a], *hyp)[0]
                    else:
                        f, t = replay(xin, W, Omega, b, theta[s][a], r[a], nd.name, nd.length, nd.scale[0], nd.nugget[0], m, omega)
                        cur[k][:, p], tol[k][:, p] = f[0], t[0]
        outs.append(cur)
        tols.append(tol)
    return outs, tols


@pytest.mark.parametrize('mode', ['dense', 'vecchia'])
@pytest.mark.parametrize('kind', ['matern2.5', 'sexp'])
def test_gp_replays_numpy(eng, kind, mode):
    """A gp with replicates and a connect column, dense and in Vecchia mode: shapes, two calls and a split of the rows give equal
    bits, the values are the numpy replay's; noise=True adds draws of variance scale * nugget (the chi-square bound of
    test_gpu_sample_paths: 6 sqrt(2 / (N - 1)) on the variance ratio); grad raises."""
    from dgp_amd import gp, kernel
    rng = np.random.default_rng(11)
    X = rng.uniform(size=(60, 3))
    X, connect = np.concatenate((X, X[:15])), np.array([2])
    Y = (np.sin(3 * X[:, 0]) + X[:, 1] * X[:, 2] + 0.05 * rng.normal(size=len(X)))[:, None]
    if mode == 'dense':
        model = _gp(kind, X, Y, connect=connect)
    else:
        model = gp(X, Y, kernel(length=np.full(3, 0.7), name=kind, scale=1.9, nugget=1e-4, input_dim=np.arange(2), connect=connect),
                   vecchia=True, m=10)
        assert model.vecch
    k = model.kernel
    J, mm = 7, 12
    np.random.seed(21)
    paths = model.sample_functions_vecchia(sample_size=J, n_features=F, m=mm)
    state = np.random.get_state()
    W, Omega, b, theta, eps = _gp_replay(model, 21, J, F)
    assert all(np.array_equal(a, c) for a, c in zip(state[1:], np.random.get_state()[1:]))   # nothing else was drawn
    assert len(W) < 75 and k.rep is not None
    y, s, eta = np.asarray(k.output, float).reshape(-1), k.scale[0], k.nugget[0]
    r = R.bracket(W, y, Omega, b, theta, eps, s, eta, k.W_diag)
    x1, x2 = rng.uniform(size=(35, 3)), rng.uniform(size=(50, 3))
    o1, o2 = paths(x1), paths(x2)
    assert o1.shape == (35, J) and o2.shape == (50, J)
    for x, o in ((x1, o1), (x2, o2)):
        ref, tol = replay(x[:, [0, 1, 2]], W, Omega, b, theta, r, kind, k.length, s, eta, mm, k.W_diag)
        within(o.T, ref, tol, 'gp %s %s' % (kind, mode))
    assert np.array_equal(paths(np.concatenate((x1, x2))), np.concatenate((o1, o2))) and np.array_equal(paths(x1), o1)
    xn = rng.uniform(size=(600, 3))
    d = (paths(xn, noise=True) - paths(xn)).reshape(-1)
    assert abs(d.var(ddof=1) / (s * eta) - 1.0) <= 6 * np.sqrt(2.0 / (d.size - 1))
    for f in (paths.grad, paths.value_and_grad):
        with pytest.raises(NotImplementedError, match='local conditioning'):
            f(x1)


def test_emulator_in_vecchia_mode_replays_the_layer_walk(eng, monkeypatch):
    """Two layers with a connect column, Vecchia mode, N = 2, sample_size = 3, m = 10: the full_layer container, every node
    against the numpy replay at the device's own outputs of the layer below, a second call and blocks of 7 rows bit for bit;
    noise=True takes one block of normals per GP node; grad raises; sample_functions still refuses the emulator."""
    from dgp_amd import emulator, pathfun
    X, model = _model('two-connect')
    emu = emulator(model.estimate(), N=2, seed=5)
    emu.to_vecchia()
    S, J, M, mm = 2, 3, 40, 10
    x = np.random.default_rng(8).uniform(size=(M, X.shape[1]))
    with pytest.raises(NotImplementedError, match='sample_paths needs a dense emulator'):
        emu.sample_functions()
    with pytest.raises(ValueError, match='conditioning-set size m must be at least 1'):
        emu.sample_functions_vecchia(m=0)
    rng = copy.deepcopy(emu._sample_rng)
    pf = emu.sample_functions_vecchia(sample_size=J, n_features=F, m=mm)
    assert isinstance(pf, pathfun.PathFunctions)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        out = pf(x, full_layer=True)
    assert [len(a) for a in out] == [2, 1] and all(u.shape == (M, S * J) for a in out for u in a)
    last = pf(x)
    assert len(last) == 1 and np.array_equal(last[0], out[1][0])
    ref, tol = walk_ref(emu, x, rng, J, mm, forced=out)
    assert emu._sample_rng.bit_generator.state == rng.bit_generator.state   # creation drew what the replay drew
    for l in range(2):
        for k in range(len(out[l])):
            within(out[l][k], ref[l][k], tol[l][k], 'layer %d node %d' % (l + 1, k + 1))
    monkeypatch.setattr(pathfun, '_rows_per_call', lambda e, P, width: 7)
    blocked = pf(x, full_layer=True)
    assert all(np.array_equal(u, w) for a, c in zip(out, blocked) for u, w in zip(a, c))
    monkeypatch.undo()
    state = copy.deepcopy(emu._sample_rng)
    noisy = pf(x, full_layer=True, noise=True)
    for k, nd in enumerate(emu.all_layer[0]):
        z = state.standard_normal((S * J, M))
        np.testing.assert_allclose(noisy[0][k], out[0][k] + np.sqrt(nd.scale[0] * nd.nugget[0]) * z.T, rtol=0, atol=1e-13)
    for f in (pf.grad, pf.value_and_grad):
        with pytest.raises(NotImplementedError, match='local conditioning'):
            f(x)
    emu.shard = True
    with pytest.raises(NotImplementedError, match='sharded over ranks'):
        emu.sample_functions_vecchia()
    emu.shard = False


def test_every_row_in_the_set_gives_sample_functions_draws(eng):
    """m >= n on a dense emulator at nugget 1e-2, from equal generator states: the objects hold the same theta and eps, and
    b(x)^T r with N(x) = all rows is c(x, W) R^-1 r.  Bound: 10 E, E the largest difference of the two numpy formulations
    (vpathfun_ref with every row in the set, pathfun_ref's dense solve) over this model's layers, each walking on its own
    outputs.  Measured: E = 3.5e-14 and a difference of 4.5e-14 between the two objects (DESIGN I.14)."""
    from dgp_amd import dgp, kernel, combine, emulator
    rng = np.random.default_rng(6)
    K = lambda **kw: kernel(length=np.array([1.0]), name='matern2.5', nugget=1e-2, **kw)
    X = rng.uniform(size=(60, 2))
    Y = np.sin(5 * X[:, :1]) * np.cos(3 * X[:, 1:]) + 0.02 * rng.normal(size=(60, 1))
    model = dgp(X, Y, combine([K(), K()], [K(scale_est=True, connect=np.arange(2))]), seed=4)
    model.train(N=3, ess_burn=3, disable=True)
    emu = emulator(model.estimate(), N=2, seed=5)
    J, M = 3, 40
    x = np.random.default_rng(8).uniform(size=(M, 2))
    start = copy.deepcopy(emu._sample_rng)
    dense = emu.sample_functions(sample_size=J, n_features=F)
    after = copy.deepcopy(emu._sample_rng)
    emu._sample_rng = copy.deepcopy(start)
    local = emu.sample_functions_vecchia(sample_size=J, n_features=F, m=60)
    assert emu._sample_rng.bit_generator.state == after.bit_generator.state
    for key, nf in dense.nodes.items():
        assert all(bool((getattr(nf, a) == getattr(local.nodes[key], a)).all()) for a in ('Omega', 'b', 'theta'))
    od, ol = dense(x, full_layer=True), local(x, full_layer=True)
    a, _ = walk_ref(emu, x, copy.deepcopy(start), J, None)
    c, _ = walk_ref(emu, x, copy.deepcopy(start), J, 60)
    E = max(np.abs(u - w).max() for u, w in zip(a, c))
    dev = max(np.abs(u - w).max() for p, q in zip(od, ol) for u, w in zip(p, q))
    print('m >= n: numpy formulations differ by E = %.3g, the two objects by %.3g (bound 10 E)' % (E, dev))
    assert dev <= 10 * E


def test_hetero_top_evaluates(eng):
    from dgp_amd import emulator
    X, model = _model('hetero')
    emu = emulator(model.estimate(), N=2, seed=5)
    emu.to_vecchia()
    pf = emu.sample_functions_vecchia(sample_size=3, n_features=F, m=10)
    x = np.random.default_rng(8).uniform(size=(30, 1))
    out = pf(x, full_layer=True)
    assert emu.all_layer[-1][0].type == 'likelihood' and [len(a) for a in out] == [2, 1]
    assert all(u.shape == (30, 6) and np.all(np.isfinite(u)) for a in out for u in a)
    assert np.array_equal(pf(x, full_layer=True)[0][0], out[0][0])   # the GP layer is a function; the top is sampled afresh
    with pytest.raises(ValueError, match='sampled node'):
        pf.grad(x)


def test_a_singular_block_warns_once_per_call(eng):
    """Two training rows 1e-9 apart and nugget 0: rows whose set holds both need a jitter rung -- one RuntimeWarning per
    evaluation call, finite values, and the other rows' bits as without the warning."""
    from dgp_amd import gp, kernel
    rng = np.random.default_rng(3)
    X = rng.uniform(size=(40, 2))
    X[7] = X[3] + 1e-9   # (not equal: equal rows would be pooled as replicates; their correlation still rounds to 1)
    Y = np.sin(4 * X[:, :1]) + X[:, 1:]
    model = gp(X, Y, kernel(length=np.array([0.8]), name='sexp', scale=1.3, nugget=0.0), vecchia=True, m=8)
    np.random.seed(2)
    paths = model.sample_functions_vecchia(sample_size=4, n_features=F, m=8)
    x = rng.uniform(size=(50, 2))
    x[0] = X[3] + 0.01
    with pytest.warns(RuntimeWarning, match='did not factor') as rec:
        out = paths(x)
    assert len(rec) == 1 and np.all(np.isfinite(out))
    far = np.abs(x - X[3]).sum(1) > 0.8   # rows with neither twin among their 8 nearest
    assert far.sum() >= 5
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        assert np.array_equal(paths(x[far]), out[far])
