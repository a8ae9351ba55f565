"""Host-side pieces of the input gradients of function-valued posterior draws (no GPU; DESIGN I.13): the public
signatures, and the numpy restatement tests/pathgrad_ref.py, which the GPU tests compare the device against, checked here
against central differences of tests/pathfun_ref.evaluate."""
import inspect
import types

import numpy as np
import pytest

H = 1e-6
FD_BOUND = 1e-7   # of max |grad|: 25 times the 4.1e-9 met on these distributions when the formulas were written down


def case(kind, nlen, D, seed):
    """n = 40 training rows, M = 37 rows of which three are training rows, F = 200 features, P = 5 paths."""
    from dgp_amd import pathfun
    rng = np.random.default_rng(seed)
    n, M, F, P = 40, 37, 200, 5
    length = rng.uniform(0.3, 1.5, size=1 if nlen == 'one' else D)
    W, x = rng.uniform(size=(n, D)), rng.uniform(size=(M, D))
    x[[0, 17, 36]] = W[[3, 0, 39]]
    Omega, b = pathfun.features(rng, kind, length, D, F)
    theta, v = rng.normal(size=(P, F)), 30.0 * rng.normal(size=(P, n))
    return x, W, Omega, b, theta, v, kind, length, 1.7


def test_signatures():
    from dgp_amd import _lib, pathfun
    from dgp_amd.ops import Engine
    assert len(_lib.SIGNATURES['dgpamd_pathfun_grad'][1]) == len(_lib.SIGNATURES['dgpamd_pathfun_eval'][1]) + 1
    assert 'dgpamd_pathgrad_workspace' not in _lib.SIGNATURES and 'dgpamd_pathfun_grad_workspace' not in _lib.SIGNATURES
    p = inspect.signature(Engine.pathfun_grad).parameters
    assert list(p)[:10] == list(inspect.signature(Engine.pathfun_eval).parameters)[:10]
    p = inspect.signature(pathfun.PathFunctions.value_and_grad).parameters
    assert list(p) == ['self', 'x', 'full_layer'] and p['full_layer'].default is False
    assert list(inspect.signature(pathfun.PathFunctions.grad).parameters) == ['self', 'x', 'full_layer']
    assert list(inspect.signature(pathfun.GpPaths.value_and_grad).parameters) == ['self', 'x']
    assert list(inspect.signature(pathfun.GpPaths.grad).parameters) == ['self', 'x']
    assert list(inspect.signature(pathfun.NodePaths.value_and_grad).parameters) == ['self', 'e', 'x']


def test_a_sampled_node_is_refused_in_plain_words():
    from dgp_amd import pathfun
    pf = pathfun.PathFunctions.__new__(pathfun.PathFunctions)
    gp, lik = types.SimpleNamespace(type='gp'), types.SimpleNamespace(type='likelihood')
    pf.layers = [[gp, gp], [lik]]
    for call in (pf.grad, pf.value_and_grad):
        with pytest.raises(ValueError, match='a sampled node has no derivative'):
            call(np.zeros((3, 2)))


@pytest.mark.parametrize('D', [1, 3, 10])
@pytest.mark.parametrize('nlen', ['one', 'D'])
@pytest.mark.parametrize('kind', ['sexp', 'matern2.5'])
def test_grad_matches_central_differences_of_evaluate(kind, nlen, D):
    import pathfun_ref as R
    import pathgrad_ref as G
    args = case(kind, nlen, D, 100 * D + (nlen == 'D'))
    x, rest = args[0], args[1:]
    g = G.grad(*args)
    assert g.shape == (5, 37, D)
    fd = G.central(lambda xx: R.evaluate(xx, *rest), x, H)
    dev = np.abs(fd - g).max() / np.abs(g).max()
    print('%s %s D=%d: max |fd - grad| / max |grad| = %.3g' % (kind, nlen, D, dev))
    assert dev <= FD_BOUND
    tol = G.tolerance(*args)
    assert tol.shape == g.shape and np.all(tol > 0) and np.all(tol < 1e-8 * np.abs(g).max())


@pytest.mark.parametrize('kind', ['sexp', 'matern2.5'])
def test_gradient_vanishes_smoothly_on_a_training_row(kind):
    """q_d = 0 at t_d = 0 and is continuous through it: one training row alone, x on it and a hair to either side."""
    import pathgrad_ref as G
    W = np.array([[0.3, 0.6]])
    x = np.array([[0.3, 0.6], [0.3 + 1e-9, 0.6], [0.3 - 1e-9, 0.6]])
    qq = G.q(x, W, kind, np.array([0.5, 0.9]))[0]
    assert np.all(qq[0] == 0.0) and qq[1, 0] < 0.0 < qq[2, 0] and abs(qq[1, 0] + qq[2, 0]) <= 1e-20 and np.all(qq[:, 1] == 0.0)
    assert np.abs(qq).max() <= 1e-7


@pytest.mark.parametrize('kind', ['sexp', 'matern2.5'])
def test_chain_rule_of_a_two_layer_composition(kind):
    """Two first-layer nodes on (x_0, x_1), a second-layer node on (node 1, node 2, x_1): the Jacobian by pathgrad_ref.chain
    against central differences of the composed evaluate."""
    import pathfun_ref as R
    import pathgrad_ref as G
    from dgp_amd import pathfun
    rng = np.random.default_rng(7)
    n, M, F, P, Dx = 40, 37, 200, 5, 2
    X = rng.uniform(size=(n, Dx))
    x = rng.uniform(size=(M, Dx))
    x[[2, 30]] = X[[5, 11]]

    def node(W, scale):
        D = W.shape[-1]
        length = rng.uniform(0.5, 1.5, size=D)
        Omega, b = pathfun.features(rng, kind, length, D, F)
        return dict(W=W, Omega=Omega, b=b, theta=rng.normal(size=(P, F)), v=rng.normal(size=(P, n)), length=length, scale=scale)

    first = [node(X, 1.0), node(X, 0.8)]
    lat = rng.uniform(size=(n, 2))
    top = node(np.concatenate((lat, X[:, 1:]), 1), 1.3)

    def ev(nd, xx, p=None):
        a = slice(None) if p is None else slice(p, p + 1)
        return R.evaluate(xx, nd['W'], nd['Omega'], nd['b'], nd['theta'][a], nd['v'][a], kind, nd['length'], nd['scale'])

    def gr(nd, xx, p=None):
        a = slice(None) if p is None else slice(p, p + 1)
        return G.grad(xx, nd['W'], nd['Omega'], nd['b'], nd['theta'][a], nd['v'][a], kind, nd['length'], nd['scale'])

    def composed(xx):
        h = np.stack([ev(nd, xx) for nd in first], 2)   # (P, M, 2)
        return np.concatenate([ev(top, np.concatenate((h[p], xx[:, 1:]), 1), p) for p in range(P)])

    h = np.stack([ev(nd, x) for nd in first], 2)
    below = np.stack([G.scatter(gr(nd, x), [0, 1], Dx) for nd in first], 2)   # (P, M, 2, Dx)
    g = np.concatenate([gr(top, np.concatenate((h[p], x[:, 1:]), 1), p) for p in range(P)])
    J = G.chain(g, below, [0, 1], [1], Dx)
    assert J.shape == (P, M, Dx)
    fd = G.central(composed, x, H)
    dev = np.abs(fd - J).max() / np.abs(J).max()
    print('%s: max |fd - J| / max |J| = %.3g' % (kind, dev))
    assert dev <= FD_BOUND
