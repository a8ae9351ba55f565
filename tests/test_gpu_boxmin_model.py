"""paths.minimize, emulator.thompson and gp.thompson (dgp_amd/optimize.py, DESIGN I.17) on small models: the optimum against
the values and gradients that paths(x) and paths.grad(x) themselves return, against the candidates, bit-for-bit replays, the
per-path walk against the shared one (the connect indexing), the refusals, and one quality check against the numpy
restatements.  Needs an MI355X: -m gpu.

The minimiser evaluates a draw at rows of its own, (P, R, Dx): the node kernels' lane form.  paths(x) evaluates it at shared
rows, where narrow nodes take the matrix form, which sums in another order: the two agree within twice I.12's forward-error
bound of one node (pathfun_ref.tolerance), carried through the layers by the node gradients (form_bound), not bit for bit."""
import copy

import numpy as np
import pytest

import boxmin_ref as B
import pathfun_ref as Rf
import pathgrad_ref as Rg
import test_gpu_pathfun as T

pytestmark = pytest.mark.gpu
GTOL = 1e-6
KW = dict(n_starts=4, n_candidates=256)


@pytest.fixture(scope='module')
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    from dgp_amd.ops import default_engine
    return default_engine(0)


def npy(t):
    return t.detach().cpu().numpy()


def node_bound(nf, xin, p):
    """(2 x I.12's bound of path p of node paths nf at the rows xin (M, D), its own gradient there (M, D))."""
    kind, length, scale, _ = nf.hyper
    W = npy(nf.W) if nf.W.dim() == 2 else npy(nf.W[int(nf.group[p])])
    args = (xin, W, npy(nf.Omega), npy(nf.b), npy(nf.theta[p:p + 1]), npy(nf.v[p:p + 1]), kind, length, scale)
    return 2.0 * Rf.tolerance(*args)[0], Rg.grad(*args)[0]


def form_bound(obj, x, output=0):
    """(M, P): how far the lane form and the matrix form of the draws can lie apart at the rows of x -- per node twice I.12's
    bound, and below the first layer the bounds of the feeding nodes times the size of the node's gradient (first order: the
    bounds are of order 1e-14)."""
    from dgp_amd import pathfun
    if isinstance(obj, pathfun.GpPaths):
        return np.stack([node_bound(obj.node, x[:, obj.columns], p)[0] for p in range(obj.sample_size)], 1)
    hidden = obj(x, full_layer=True)
    P = obj.N * obj.sample_size
    err = []
    for l, layer in enumerate(obj.layers):
        cur = []
        for k, nd in enumerate(layer):
            e = np.empty((len(x), P))
            connect = [] if nd.connect is None else list(nd.connect)
            for p in range(P):
                if l == 0:
                    xin = x[:, list(nd.input_dim) + connect]
                else:
                    xin = np.concatenate([np.stack([hidden[l - 1][int(i)][:, p] for i in nd.input_dim], 1), x[:, connect]], 1)
                tol, g = node_bound(obj.nodes[l, k], np.ascontiguousarray(xin), p)
                e[:, p] = tol
                if l:
                    e[:, p] += sum(np.abs(g[:, i]) * err[l - 1][int(kk)][:, p] for i, kk in enumerate(nd.input_dim))
            cur.append(e)
        err.append(cur)
    return err[-1][output]


def own(a):
    """Entry [p] of path p from an (M = P, P) array."""
    return np.diagonal(a).copy()


def values_of(obj, x, output=0):
    out = obj(x)
    return out if isinstance(out, np.ndarray) else out[output]


def grads_of(obj, x, output=0):
    g = obj.grad(x)
    return g if isinstance(g, np.ndarray) else g[output]


def same(a, c):
    return all(np.array_equal(getattr(a, n), getattr(c, n)) for n in ('x0', 'x', 'fun', 'x_all', 'fun_all', 'status', 'n_iter', 'n_eval', 'start'))


def check_optimum(obj, bounds, res, seed, output=0):
    """What every result must satisfy, against the draws' own shared-rows evaluation."""
    from dgp_amd import optimize
    P, Dx = res.x.shape
    lo, hi = bounds[:, 0], bounds[:, 1]
    R = res.x_all.shape[1]
    assert res.fun.shape == (P,) and res.x_all.shape == (P, R, Dx) and res.start.shape == (P,) and res.success.shape == (P,)
    assert all(getattr(res, n).shape == (P, R) for n in ('fun_all', 'status', 'n_iter', 'n_eval'))
    assert np.all(res.x_all >= lo) and np.all(res.x_all <= hi)
    assert np.all((res.status >= 1) & (res.status <= 6)) and np.all(res.n_eval <= res.rounds)
    rows = np.arange(P)
    assert np.array_equal(res.fun, res.fun_all[rows, res.start]) and np.array_equal(res.fun, res.fun_all.min(1))
    # the value: the draw's own, as paths(x) gives it at the same point
    slack = own(form_bound(obj, res.x, output))
    diff = np.abs(res.fun - own(values_of(obj, res.x, output)))
    print('fun against paths(x): largest difference / bound %.3g' % np.max(diff / slack))
    assert np.all(diff <= slack)
    # the point: a Karush-Kuhn-Tucker point by the gradient that paths.grad returns
    g = np.stack([grads_of(obj, res.x, output)[p, :, p] for p in range(P)])
    kkt = np.array([B.kkt(res.x[p], g[p], lo, hi) for p in range(P)])
    print('successful paths %d of %d; largest residual %.3g' % (res.success.sum(), P, kkt[res.success].max(initial=0.0)))
    assert res.success.sum() >= 1 and np.all(kkt[res.success] <= 2 * GTOL)
    summ = res.summary(0.9)
    assert summ['x']['mean'].shape == (Dx,) and np.all(summ['x']['lower'] <= summ['x']['upper']) and summ['fun']['lower'] <= summ['fun']['upper']
    if seed is not None:   # no worse than the best candidate (the starts are the best candidates, and no accepted step goes up)
        cand = optimize.candidates(lo, hi, KW['n_candidates'], seed)
        fc = values_of(obj, cand, output)
        best = np.argmin(fc, 0)
        slack = own(form_bound(obj, cand[best], output))
        assert np.all(res.fun <= fc[best, rows] + slack)
        order = np.argsort(fc, 0, kind='stable')[:R].T
        assert np.array_equal(res.x0, cand[order])


# ------------------------------------------------------------------------------------------------ gp
def bowl(n=40):
    rng = np.random.default_rng(12)
    X = rng.uniform(size=(n, 2))
    return X, ((X[:, 0] - 0.3) ** 2 + (X[:, 1] - 0.6) ** 2)[:, None]


BOX = np.array([[0.0, 1.0], [0.0, 1.0]])


@pytest.fixture(scope='module')
def gp_paths(eng):
    X, Y = bowl()
    m = T._gp('sexp', X, Y)
    np.random.seed(31)
    return m, m.sample_functions(sample_size=6, n_features=128)


def test_gp_minimize(eng, gp_paths):
    m, paths = gp_paths
    res = paths.minimize(BOX, seed=3, **KW)
    check_optimum(paths, BOX, res, 3)
    assert same(res, paths.minimize(BOX, seed=3, **KW))          # the same arguments: the same bits
    # the draws follow the bowl: their minimisers gather around (0.3, 0.6)
    assert np.all(np.abs(np.median(res.x, 0) - np.array([0.3, 0.6])) < 0.2)
    q = paths.minimize(BOX, seed=3, qmc=True, **KW)
    assert q.x.shape == res.x.shape and np.all(q.x >= 0.0) and np.all(q.x <= 1.0)


def test_gp_starts_prefix_and_blocks(eng, gp_paths, monkeypatch):
    from dgp_amd import pathfun
    m, paths = gp_paths
    x0 = np.random.default_rng(4).uniform(size=(4, 2))
    four, two = paths.minimize(BOX, x0=x0), paths.minimize(BOX, x0=x0[:2])
    for n in ('x_all', 'fun_all', 'status', 'n_iter', 'n_eval'):   # a problem does not depend on the problems beside it
        assert np.array_equal(getattr(four, n)[:, :2], getattr(two, n))
    per_path = paths.minimize(BOX, x0=np.broadcast_to(x0, (6, 4, 2)).copy())
    assert same(per_path, four)
    whole = paths.minimize(BOX, seed=5, **KW)
    for rows in (7, 64, 200):
        monkeypatch.setattr(pathfun, '_rows_per_call', lambda e, P, width, rows=rows: rows)
        assert same(paths.minimize(BOX, seed=5, **KW), whole)


def test_gp_maximize_is_minimize_of_the_negated_draw(eng, gp_paths):
    m, paths = gp_paths
    x0 = np.random.default_rng(6).uniform(size=(4, 2))
    neg = copy.copy(paths)
    neg.node = copy.copy(paths.node)
    neg.node.theta, neg.node.v = -paths.node.theta, -paths.node.v   # (the draw is linear in them: every bit but the sign stays)
    assert np.array_equal(neg(x0), -paths(x0))
    up, down = paths.minimize(BOX, x0=x0, maximize=True), neg.minimize(BOX, x0=x0)
    for n in ('x_all', 'status', 'n_iter', 'n_eval', 'x', 'start'):
        assert np.array_equal(getattr(up, n), getattr(down, n))
    assert np.array_equal(up.fun_all, -down.fun_all) and np.array_equal(up.fun, up.fun_all.max(1))


def test_gp_thompson_and_refusals(eng, gp_paths):
    from dgp_amd import gp, kernel
    m, paths = gp_paths
    np.random.seed(8)
    X_new, res = m.thompson(BOX, batch_size=5, n_features=64, seed=2, **KW)
    assert X_new.shape == (5, 2) and res.x.shape == (5, 2) and np.array_equal(X_new, res.x)
    assert np.all(X_new >= 0.0) and np.all(X_new <= 1.0)
    np.random.seed(8)
    again, _ = m.thompson(BOX, batch_size=5, n_features=64, seed=2, **KW)
    assert np.array_equal(again, X_new)
    for bad in (BOX[0], BOX[:1], np.array([[0.0, 1.0], [np.nan, 1.0]]), np.array([[0.0, 1.0], [1.0, 0.5]]), BOX.T[:, :1]):
        with pytest.raises(ValueError):
            paths.minimize(bad, **KW)
    for kw in (dict(output=1), dict(output=-1), dict(n_starts=0), dict(n_candidates=2), dict(maxiter=0), dict(history=17),
               dict(gtol=-1.0), dict(x0=np.zeros((3, 4, 2))), dict(x0=np.zeros((4, 3))), dict(qmc=True, n_candidates=100)):
        with pytest.raises(ValueError):
            paths.minimize(BOX, **dict(KW, **kw))
    with pytest.raises(ValueError):
        m.thompson(BOX, batch_size=0)
    X, Y = bowl()
    np.random.seed(1)
    local = m.sample_functions_vecchia(sample_size=2, n_features=16, m=10)
    with pytest.raises(NotImplementedError, match='sample_functions '):
        local.minimize(BOX, **KW)
    vg = gp(X, Y, kernel(length=np.array([0.5]), name='sexp'), vecchia=True, m=10)
    with pytest.raises(NotImplementedError):
        vg.thompson(BOX)


# ------------------------------------------------------------------------------------------------ the quality check
QUALITY_SEED = 17     # (chosen on the CPU: tests/test_boxmin_host.py::test_quality_seed holds the restatement to scipy on it)
QUALITY = dict(J=6, F=96, R=4, candidates=256)


def quality_case(seed=QUALITY_SEED):
    """The fixed-hyperparameter gp of this file and its draws under np.random.seed(seed), in numpy: (funs[p](x) -> (value,
    gradient) of draw p, the starts x0 (R, 2), each draw's spread over the candidate rows (J,))."""
    import types
    X, Y = bowl()
    kind, length, scale, nugget = 'sexp', np.full(2, 0.7), 1.9, 1e-4
    k = types.SimpleNamespace(name=kind, length=length, _X=lambda: X)
    _, Omega, b, theta, eps = T._gp_replay(types.SimpleNamespace(kernel=k), seed, QUALITY['J'], QUALITY['F'])
    v = Rf.weights(X, Y[:, 0], Omega, b, theta, eps, kind, length, scale, nugget, None)
    funs = [lambda x, p=p: (float(Rf.evaluate(x[None], X, Omega, b, theta[p:p + 1], v[p:p + 1], kind, length, scale)[0, 0]),
                            Rg.grad(x[None], X, Omega, b, theta[p:p + 1], v[p:p + 1], kind, length, scale)[0, 0])
            for p in range(QUALITY['J'])]
    rng = np.random.default_rng(seed)
    cand = rng.uniform(size=(QUALITY['candidates'], 2))
    fc = Rf.evaluate(cand, X, Omega, b, theta, v, kind, length, scale)
    return funs, rng.uniform(size=(QUALITY['R'], 2)), fc.max(1) - fc.min(1)


def quality_best(funs, x0, minimiser):
    """Each draw's best value over the starts."""
    return np.array([min(minimiser(f, s) for s in x0) for f in funs])


def test_device_finds_the_restatements_optima(eng):
    """Every draw's best value over four starts agrees with the numpy restatement's (boxmin_ref on pathfun_ref / pathgrad_ref,
    the same generator draws, the same starts) within 1e-6 of the draw's spread over the candidate rows; no path is left out."""
    funs, x0, spread = quality_case()
    X, Y = bowl()
    m = T._gp('sexp', X, Y)
    np.random.seed(QUALITY_SEED)
    paths = m.sample_functions(sample_size=QUALITY['J'], n_features=QUALITY['F'])
    res = paths.minimize(BOX, x0=x0)
    ref = quality_best(funs, x0, lambda f, s: B.minimize(f, s, BOX[:, 0], BOX[:, 1])['fun'])
    print('device against the restatement: largest |difference| / spread %.3g (1e-6)' % np.max(np.abs(res.fun - ref) / spread))
    assert np.all(np.abs(res.fun - ref) <= 1e-6 * spread)


# ------------------------------------------------------------------------------------------------ emulators
@pytest.fixture(scope='module', params=['two-connect', 'three'])
def emu_paths(request, eng):
    from dgp_amd import emulator
    X, model = T._model(request.param)
    emu = emulator(model.estimate(), N=2, seed=5)
    return request.param, emu, emu.sample_functions(sample_size=3, n_features=100)


def test_per_path_walk_is_the_shared_walk(eng, emu_paths):
    """The walk at xd.expand(P, M, Dx) -- every path at rows of its own, here all the same -- against the walk at xd: a deeper
    node's `connect` columns index the per-path input as they index the shared one ('two-connect': columns 0 and 1 of x feed
    the second layer beside the two hidden outputs)."""
    which, emu, paths = emu_paths
    x = np.random.default_rng(9).uniform(size=(11, 2))
    xd = paths.engine.tensor(x)
    P = emu.N * 3
    shared = [(npy(c), npy(J)) for c, J in paths._walk(xd, jacobians='all')]
    lanes = [(npy(c), npy(J)) for c, J in paths._walk(xd[None].expand(P, 11, 2).contiguous(), jacobians='all')]
    bound = form_bound(paths, x).T
    diff = np.abs(lanes[-1][0][:, :, 0] - shared[-1][0][:, :, 0])
    print('%s: per-path walk against shared walk, largest difference / bound %.3g' % (which, np.max(diff / bound)))
    assert np.all(diff <= bound)
    scale = np.max(np.abs(shared[-1][1]))
    assert np.max(np.abs(lanes[-1][1] - shared[-1][1])) <= 1e-9 * scale      # (the Jacobians: the same chain rule, far from a wrong column)
    if which == 'two-connect':
        assert np.max(np.abs(shared[-1][1])) > 0 and emu.all_layer[1][0].connect is not None


def test_emulator_minimize_and_thompson(eng, emu_paths):
    which, emu, paths = emu_paths
    res = paths.minimize(BOX, seed=7, **KW)
    check_optimum(paths, BOX, res, 7)
    assert same(res, paths.minimize(BOX, seed=7, **KW))
    up = paths.minimize(BOX, seed=7, maximize=True, **KW)
    assert np.all(up.fun >= res.fun) and np.array_equal(up.fun, up.fun_all.max(1))
    state = copy.deepcopy(emu._sample_rng)
    X_new, all_draws = emu.thompson(BOX, batch_size=3, n_features=64, seed=1, **KW)     # N = 2: two draws per imputation
    assert X_new.shape == (3, 2) and all_draws.x.shape == (4, 2) and np.all(X_new >= 0.0) and np.all(X_new <= 1.0)
    assert np.array_equal(X_new, all_draws.x[[0, 2, 1]])                                 # row b: path (b mod N) J + b div N
    emu._sample_rng = state
    assert np.array_equal(emu.thompson(BOX, batch_size=3, n_features=64, seed=1, **KW)[0], X_new)
    with pytest.raises(ValueError):
        paths.minimize(BOX, output=1, **KW)
    with pytest.raises(ValueError):
        paths.minimize(BOX[:1], **KW)


def test_sampled_nodes_are_refused(eng):
    from dgp_amd import emulator
    X, model = T._model('hetero')
    emu = emulator(model.estimate(), N=2, seed=5)
    with pytest.raises(ValueError, match='sampled node'):
        emu.sample_functions(sample_size=2, n_features=16).minimize(np.array([[0.0, 1.0]]), **KW)
    with pytest.raises(ValueError, match='sampled node'):
        emu.thompson(np.array([[0.0, 1.0]]), batch_size=2, n_features=16, **KW)
    _, model = T._model('two-connect', 'sexp')
    emu = emulator(model.estimate(), N=2, seed=1)
    with pytest.raises(NotImplementedError, match='sample_functions '):
        emu.sample_functions_vecchia(sample_size=2, n_features=16, m=10).minimize(BOX, **KW)
    emu.to_vecchia()
    with pytest.raises(NotImplementedError, match='dense emulator'):
        emu.thompson(BOX)
