"""Input gradients of function-valued posterior draws (dgpamd_pathfun_grad, paths.grad, paths.value_and_grad; DESIGN
I.13).  Needs an MI355X: -m gpu.

The reference is the numpy restatement tests/pathgrad_ref.py; the tolerance of a gradient is its forward-error bound
(pathgrad_ref.tolerance), computed from the inputs of each case.  The values that come with the gradients are compared with
dgpamd_pathfun_eval's bit for bit.  Every comparison prints the largest error / bound it met before it asserts."""
import numpy as np
import pytest

from far_ref import FAR_SCALE, far_inputs

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


def features_for(kind, length, D, F, seed):
    from dgp_amd import pathfun
    return pathfun.features(np.random.default_rng(seed), kind, length, D, F)


def check_operator(eng, kind, length, n, D, F, P, M, shape, seed, groups=1, x=None, W=None, what='', scale=1.7):
    """One call of pathfun_grad against the restatement, and its values against pathfun_eval's bits.  shape 'shared': x
    (M, D) and one training set; 'per-path': x (P, M, D) and `groups` training sets in mixed order."""
    import torch
    import pathgrad_ref as G
    rng = np.random.default_rng(seed)
    Omega, b = features_for(kind, length, D, F, seed + 1)
    if W is None:
        W = rng.uniform(size=(groups, n, D))
    theta, v = rng.normal(size=(P, F)), rng.normal(size=(P, n))
    group = rng.integers(0, groups, size=P) if shape == 'per-path' else np.zeros(P, dtype=int)
    if x is None:
        x = rng.uniform(size=(M, D) if shape == 'shared' else (P, M, D))
    t = eng.tensor
    args = (kind, t(x), t(W[0] if shape == 'shared' else W) if n else None, t(Omega), t(b), t(theta), t(v) if n else None, length,
            scale)
    kw = dict(group=group) if shape == 'per-path' else {}
    out, grad = eng.pathfun_grad(*args, **kw)
    assert out.shape == (P, M) and grad.shape == (P, M, D)
    assert torch.equal(out, eng.pathfun_eval(*args, **kw)), what + ': the values are not pathfun_eval\'s'
    grad = npy(grad)
    assert np.all(np.isfinite(grad))
    worst = 0.0
    for p in range(P):
        a = slice(p, p + 1)
        xp, Wp = (x if shape == 'shared' else x[p]), (W[group[p]] if n else None)
        ref = G.grad(xp, Wp, Omega, b, theta[a], v[a] if n else None, kind, length, scale)
        tol = G.tolerance(xp, Wp, Omega, b, theta[a], v[a] if n else None, kind, length, scale)
        ratio = float((np.abs(grad[a] - ref) / tol).max())
        assert ratio <= 1.0, (what, shape, 'path', p, ratio)
        worst = max(worst, ratio)
    print('%s %s: max error / bound = %.3g' % (what, shape, worst))
    return worst


# ------------------------------------------------------------------------------------------------ operator
@pytest.mark.parametrize('n', [1, 63, 64, 65, 200])
@pytest.mark.parametrize('nlen', ['one', 'D'])
@pytest.mark.parametrize('kind', ['sexp', 'matern2.5'])
def test_grad_matches_the_restatement(eng, kind, nlen, n):
    """Shared inputs (the matrix form) and per-path inputs over two groups (the lane form), across the 64-row staging tile."""
    length = np.array([0.8]) if nlen == 'one' else np.array([0.6, 1.1, 0.4])
    what = '%s %s n=%d' % (kind, nlen, n)
    check_operator(eng, kind, length, n, 3, 33, 5, 70, 'shared', 10 * n, what=what)
    check_operator(eng, kind, length, n, 3, 33, 5, 257, 'per-path', 10 * n + 5, groups=2, what=what)


@pytest.mark.parametrize('D', [1, 2, 3, 5, 6, 7, 10, 11, 16, 17, 33, 64])
@pytest.mark.parametrize('kind', ['sexp', 'matern2.5'])
def test_grad_at_every_compiled_width_and_its_neighbours(eng, kind, D):
    """Widths 2, 4, 6, 8, 10, 16, 32, 64 are compiled; shared x takes the matrix form up to 10 columns and the lane form from
    11 on."""
    length = np.sqrt(D) * np.random.default_rng(D).uniform(0.5, 1.2, size=D)
    for shape in ('shared', 'per-path'):
        check_operator(eng, kind, length, 40, D, 40, 3, 70, shape, 100 + D, what='%s D=%d' % (kind, D))


@pytest.mark.parametrize('P', [1, 64, 65, 129, 300])
def test_grad_over_many_paths(eng, P):
    """More paths than one workgroup's 64 columns (shared inputs) and than one launch's 64 groups (per-path inputs)."""
    length = np.array([0.7])
    check_operator(eng, 'matern2.5', length, 33, 5, 65, P, 65, 'shared', P, what='P=%d' % P)
    check_operator(eng, 'matern2.5', length, 33, 5, 65, P, 65, 'per-path', P + 1, groups=3, what='P=%d' % P)


@pytest.mark.parametrize('F', [1, 31, 32, 33, 64, 65])
@pytest.mark.parametrize('kind', ['sexp', 'matern2.5'])
def test_grad_of_the_prior_part_alone(eng, kind, F):
    """n = 0, across the 32- and 64-feature staging tiles."""
    length = np.array([0.6, 1.1, 0.9])
    for shape in ('shared', 'per-path'):
        check_operator(eng, kind, length, 0, 3, F, 3, 70, shape, F, what='%s n=0 F=%d' % (kind, F))


@pytest.mark.parametrize('kind', ['sexp', 'matern2.5'])
def test_grad_on_training_rows_and_with_large_arguments(eng, kind):
    """Rows equal to training rows (t_d = 0: q_d = 0, what is left is the rounding of x_d / g_d and W_id / g_d), and a
    lengthscale of 0.002: |Omega . x + b| in the hundreds."""
    rng = np.random.default_rng(3)
    n, D, P = 40, 3, 3
    W = rng.uniform(size=(1, n, D))
    length = np.array([0.6, 1.1, 0.9])
    check_operator(eng, kind, length, n, D, 40, P, n, 'shared', 1, x=W[0].copy(), W=W, what=kind + ' on training rows')
    xs = np.stack([W[0][rng.permutation(n)] for _ in range(P)])
    check_operator(eng, kind, length, n, D, 40, P, n, 'per-path', 2, x=xs, W=W, what=kind + ' on training rows')
    short = np.array([0.6, 0.002, 0.9])
    Omega, b = features_for(kind, short, D, 64, 9)
    x = rng.uniform(size=(70, D))
    assert np.abs(x @ Omega.T + b).max() > 300.0
    for shape in ('shared', 'per-path'):
        check_operator(eng, kind, short, n, D, 64, P, 70, shape, 8, what=kind + ' length 0.002')


@pytest.mark.parametrize('s', [1.0, 1e4])
@pytest.mark.parametrize('kind', ['sexp', 'matern2.5'])
def test_grad_beyond_the_exponent_range(eng, kind, s):
    """n = 65 training rows and M = 70 rows of far_inputs (the first 65 ARE training rows: c = 1 and q = 0 there, c = 0 on every
    other pair), shared and per-path x.  With random theta: check_operator's bound (and pathfun_eval's bits).  With theta = 0 only
    the correlation part is left and the restatement's gradient is exactly 0 everywhere: here it may be 1e-300 at the most, and
    the values are v[p, m] sqrt(scale) on the training rows within pathfun_ref's bound and at most 1e-300 on the others."""
    import pathfun_ref as R
    import pathgrad_ref as G
    n, M, D, F, P, scale = 65, 70, 2, 64, 3, FAR_SCALE
    length = np.array([1e-5])
    W, x = far_inputs(n, s)[None], far_inputs(M, s)
    xs = np.stack([x, x[::-1].copy(), np.roll(x, 3, axis=0)])
    what = '%s s=%g' % (kind, s)
    check_operator(eng, kind, length, n, D, F, P, M, 'shared', 11, x=x, W=W, what=what, scale=scale)
    check_operator(eng, kind, length, n, D, F, P, M, 'per-path', 12, x=xs, W=W, what=what, scale=scale)
    Omega, b = features_for(kind, length, D, F, 13)
    theta, v = np.zeros((P, F)), np.random.default_rng(14).normal(size=(P, n))
    t = eng.tensor
    for shape, xx in (('shared', x), ('per-path', xs)):
        out, grad = eng.pathfun_grad(kind, t(xx), t(W[0]), t(Omega), t(b), t(theta), t(v), length, scale)
        out, grad = npy(out), npy(grad)
        for p in range(P):
            a, xp = slice(p, p + 1), (xx if shape == 'shared' else xx[p])
            with np.errstate(invalid='ignore'):
                gref = G.grad(xp, W[0], Omega, b, theta[a], v[a], kind, length, scale)
            assert not gref.any()
            assert np.all(np.abs(grad[a]) <= 1e-300), (what, shape, p, np.abs(grad[a]).max())
            ref = R.evaluate(xp, W[0], Omega, b, theta[a], v[a], kind, length, scale)
            z = ref == 0.0
            assert z.sum() == M - n and np.all(np.abs(out[a][z]) <= 1e-300), (what, shape, p)
            tol = R.tolerance(xp, W[0], Omega, b, theta[a], v[a], kind, length, scale)
            within(out[a][~z], ref[~z], tol[~z], '%s %s theta 0 path %d' % (what, shape, p))


@pytest.mark.parametrize('shape', ['shared', 'per-path'])
@pytest.mark.parametrize('D', [4, 12])
def test_rows_are_independent_bit_for_bit(eng, shape, D):
    """One call at 1000 rows equals the same rows in the slices [0:1], [1:65], [65:1000], values and gradients (D = 4: the
    matrix form for shared inputs; D = 12: the lane form for both)."""
    import torch
    rng = np.random.default_rng(5)
    kind, n, M, F, scale = 'matern2.5', 70, 1000, 100, 1.1
    P = 70 if shape == 'shared' else 3
    length = rng.uniform(0.5, 1.5, size=D)
    Omega, b = features_for(kind, length, D, F, 9)
    t = eng.tensor
    W, theta, v = t(rng.uniform(size=(n, D))), t(rng.normal(size=(P, F))), t(rng.normal(size=(P, n)))
    Om, bd = t(Omega), t(b)
    x = t(rng.uniform(size=(M, D)) if shape == 'shared' else rng.uniform(size=(P, M, D)))
    full, gfull = eng.pathfun_grad(kind, x, W, Om, bd, theta, v, length, scale)
    again, gagain = eng.pathfun_grad(kind, x, W, Om, bd, theta, v, length, scale)
    assert torch.equal(full, again) and torch.equal(gfull, gagain)
    cuts = [0, 1, 65, M]
    parts = [eng.pathfun_grad(kind, x[..., a:c, :].contiguous(), W, Om, bd, theta, v, length, scale) for a, c in zip(cuts, cuts[1:])]
    assert torch.equal(full, torch.cat([pt[0] for pt in parts], 1))
    assert torch.equal(gfull, torch.cat([pt[1] for pt in parts], 1))
    assert bool(torch.isfinite(gfull).all())


def test_grad_refuses_what_it_cannot_do(eng):
    from dgp_amd.ops import DgpAmdError
    rng = np.random.default_rng(0)
    t = eng.tensor
    x, W, Om, b = rng.uniform(size=(4, 2)), rng.uniform(size=(2, 6, 2)), rng.normal(size=(8, 2)), rng.uniform(size=8)
    th, v = rng.normal(size=(3, 8)), rng.normal(size=(3, 6))
    with pytest.raises(DgpAmdError, match='one group'):   # shared inputs and two training sets
        eng.pathfun_grad('sexp', t(x), t(W), t(Om), t(b), t(th), t(v), [1.0], 1.0, group=[0, 1, 0])
    with pytest.raises(DgpAmdError, match='out of range'):
        eng.pathfun_grad('sexp', t(np.stack([x] * 3)), t(W), t(Om), t(b), t(th), t(v), [1.0], 1.0, group=[0, 2, 0])
    with pytest.raises(DgpAmdError, match='bad D / nlen'):
        eng.pathfun_grad('sexp', t(x), t(W[0]), t(Om), t(b), t(th), t(v), [1.0, 1.0, 1.0], 1.0)
    with pytest.raises(DgpAmdError, match='non-negative'):
        eng.pathfun_grad('sexp', t(x), t(W[0]), t(Om), t(b), t(th), t(v), [1.0], -1.0)


# ------------------------------------------------------------------------------------------------ gp
@pytest.mark.parametrize('case', ['matern2.5-replicates-connect', 'sexp-plain'])
def test_gp_grad_matches_the_restatement_on_its_own_arrays(eng, case):
    import pathgrad_ref as G
    from test_gpu_pathfun import _gp
    kind = case.split('-')[0]
    rng = np.random.default_rng(11)
    X = rng.uniform(size=(60, 3))
    connect = None
    if 'replicates' in case:
        X, connect = np.concatenate((X, X[:15])), np.array([2])
    Y = (np.sin(3 * X[:, 0]) + X[:, 1] * X[:, 2] + 0.05 * rng.normal(size=len(X)))[:, None]
    m = _gp(kind, X, Y, connect=connect)
    J, F, M, Dx = 7, 256, 35, 5
    np.random.seed(21)
    paths = m.sample_functions(sample_size=J, n_features=F)
    nf = paths.node
    cols = np.arange(3) if connect is None else np.concatenate((np.setdiff1d(np.arange(3), connect), connect))
    x = rng.uniform(size=(M, Dx))   # columns 3 and 4 are not read by the model
    x[:4, :3] = X[:4]
    vals, grad = paths.value_and_grad(x)
    assert vals.shape == (M, J) and grad.shape == (M, Dx, J)
    assert np.array_equal(vals, paths(x)) and np.array_equal(grad, paths.grad(x))
    assert np.all(grad[:, 3:, :] == 0.0)
    kind_, length, scale, _ = nf.hyper
    arrays = [npy(a) for a in (nf.W, nf.Omega, nf.b, nf.theta, nf.v)]
    ref = G.scatter(G.grad(x[:, cols], *arrays, kind_, length, scale), cols, Dx)
    tol = G.scatter(G.tolerance(x[:, cols], *arrays, kind_, length, scale), cols, Dx)
    used = np.sort(cols)
    within(grad.transpose(2, 0, 1)[:, :, used], ref[:, :, used], tol[:, :, used], 'gp %s' % case)


# ------------------------------------------------------------------------------------------------ emulator
_MODELS = {}


def model(which):
    from test_gpu_pathfun import _model
    if which not in _MODELS:
        _MODELS[which] = _model(which)
    return _MODELS[which]


def replay(pf, x, vals):
    """The walk's chain rule in numpy on the nodes' own arrays, at the device's own outputs of the layer below:
    per layer (Jacobian, bound), each (P, M, K, Dx).

    The bound.  A node's computed gradient is g + dg with |dg| <= tg (pathgrad_ref.tolerance at the inputs the device used),
    the computed Jacobian of the layer below Jb + dJ with |dJ| <= Tb.  The device forms sum_k (g_k + dg_k)(Jb_k + dJ_k) by
    one fused multiply-add per k (each rounds the running sum once: at most (kd + 1) eps sum_k |g_k| |Jb_k| over the kd
    terms) and adds the connect part (one rounding per column, eps |J|, and that part's own tg):
        T = sum_k ( tg_k |Jb_k| + (|g_k| + tg_k) Tb_k ) + (kd + 1) eps sum_k |g_k| |Jb_k| + scatter(tg_connect) + eps |J|.
    A first-layer Jacobian is the node's gradient scattered into x's columns: T = scatter(tg)."""
    import pathgrad_ref as G
    P, M, Dx = pf.N * pf.sample_size, len(x), x.shape[1]
    out = []
    for l, layer in enumerate(pf.layers):
        Jl, Tl = np.zeros((P, M, len(layer), Dx)), np.zeros((P, M, len(layer), Dx))
        for k, nd in enumerate(layer):
            nf = pf.nodes[l, k]
            kind, length, scale, _ = nf.hyper
            W, Omega, b, theta, v = [npy(a) for a in (nf.W, nf.Omega, nf.b, nf.theta, nf.v)]
            connect = [] if nd.connect is None else list(nd.connect)
            if l == 0:
                cols = list(nd.input_dim) + connect
                Jl[:, :, k] = G.scatter(G.grad(x[:, cols], W, Omega, b, theta, v, kind, length, scale), cols, Dx)
                Tl[:, :, k] = G.scatter(G.tolerance(x[:, cols], W, Omega, b, theta, v, kind, length, scale), cols, Dx)
                continue
            kd = len(nd.input_dim)
            g, tg = np.empty((P, M, kd + len(connect))), np.empty((P, M, kd + len(connect)))
            for p in range(P):
                a = slice(p, p + 1)
                xin = np.stack([vals[l - 1][kk][:, p] for kk in nd.input_dim], 1)
                if connect:
                    xin = np.concatenate((xin, x[:, connect]), 1)
                g[a] = G.grad(xin, W[nf.group[p]], Omega, b, theta[a], v[a], kind, length, scale)
                tg[a] = G.tolerance(xin, W[nf.group[p]], Omega, b, theta[a], v[a], kind, length, scale)
            Jb, Tb = out[l - 1][0][:, :, list(nd.input_dim)], out[l - 1][1][:, :, list(nd.input_dim)]
            Jl[:, :, k] = G.chain(g, out[l - 1][0], nd.input_dim, nd.connect, Dx)
            gk, tk = np.abs(g[..., :kd, None]), tg[..., :kd, None]
            Tl[:, :, k] = (tk * np.abs(Jb) + (gk + tk) * Tb + (kd + 1) * G.EPS * gk * np.abs(Jb)).sum(2) + \
                G.scatter(tg[..., kd:], connect, Dx) + G.EPS * np.abs(Jl[:, :, k])
        out.append((Jl, Tl))
    return out


@pytest.mark.parametrize('which', ['two-connect', 'three'])
def test_emulator_grad_replays_the_chain_rule(eng, which, monkeypatch):
    from dgp_amd import emulator, pathfun
    X, mdl = model(which)
    emu = emulator(mdl.estimate(), N=2, seed=5)
    S, J, F, M, Dx = 2, 3, 200, 40, X.shape[1] + 1
    x = np.random.default_rng(8).uniform(size=(M, Dx))   # the last column is not read by the model
    x[:3, :X.shape[1]] = X[:3]
    pf = emu.sample_functions(sample_size=J, n_features=F)
    vals, grads = pf.value_and_grad(x, full_layer=True)
    ref_vals = pf(x, full_layer=True)
    assert len(vals) == len(ref_vals) == len(grads) == emu.n_layer
    for a, c, g in zip(vals, ref_vals, grads):
        assert len(a) == len(c) == len(g)
        assert all(np.array_equal(u, w) and u.shape == (M, S * J) for u, w in zip(a, c))
        assert all(u.shape == (M, Dx, S * J) and np.all(u[:, -1] == 0.0) for u in g)
    last_vals, last = pf.value_and_grad(x)
    assert all(np.array_equal(u, w) for u, w in zip(last, grads[-1])) and all(np.array_equal(u, w) for u, w in zip(last_vals, vals[-1]))
    assert all(np.array_equal(u, w) for u, w in zip(pf.grad(x), grads[-1]))
    for l, (Jl, Tl) in enumerate(replay(pf, x, vals)):
        for k in range(Jl.shape[2]):
            used = np.abs(Jl[:, :, k]).max((0, 1)) > 0
            assert not used[-1]
            within(grads[l][k].transpose(2, 0, 1)[:, :, used], Jl[:, :, k][:, :, used], Tl[:, :, k][:, :, used],
                   '%s layer %d node %d' % (which, l + 1, k + 1))
            assert np.all(grads[l][k][:, ~used] == 0.0)
    # a forced small row block changes no bit
    monkeypatch.setattr(pathfun, '_rows_per_call', lambda e, P, width: 7)
    v2, g2 = pf.value_and_grad(x, full_layer=True)
    for a, c in zip(vals + grads, v2 + g2):
        assert all(np.array_equal(u, w) for u, w in zip(a, c))


def test_grad_against_central_differences_of_the_public_paths(eng):
    """paths(x) is a deterministic function of x: central differences of it at h = 1e-6 against paths.grad(x), within
    1e-6 max |grad|, on a two-layer model with a `connect` column.  Central differences lose eps |v| / h to cancellation
    whatever is differentiated, so the model has a nugget of 1e-2 (moderate weights v); that the differences are then good
    enough is checked first, on the numpy replay of the same composition alone (float64 evaluate and the chain rule on the
    nodes' own arrays, nothing from the device): within 1e-7 max |J|."""
    import pathfun_ref as R
    import pathgrad_ref as G
    from dgp_amd import combine, dgp, emulator, kernel
    rng = np.random.default_rng(6)
    X = rng.uniform(size=(60, 2))
    Y = np.sin(5 * X[:, :1]) * np.cos(3 * X[:, 1:]) + 0.02 * rng.normal(size=(60, 1))
    K = lambda **kw: kernel(length=np.array([1.0]), name='matern2.5', nugget=1e-2, **kw)
    mdl = dgp(X, Y, combine([K(), K()], [K(scale_est=True, connect=np.arange(2))]), seed=4)
    mdl.train(N=3, ess_burn=3, disable=True)
    emu = emulator(mdl.estimate(), N=2, seed=5)
    pf = emu.sample_functions(sample_size=3, n_features=200)
    P, h = 6, 1e-6
    x = np.random.default_rng(12).uniform(0.05, 0.95, size=(30, 2))

    def composed(xx, container=False):
        vals = []
        for l, layer in enumerate(pf.layers):
            cur = np.empty((P, len(xx), len(layer)))
            for k, nd in enumerate(layer):
                nf = pf.nodes[l, k]
                kind, length, scale, _ = nf.hyper
                W, Omega, b, theta, v = [npy(a) for a in (nf.W, nf.Omega, nf.b, nf.theta, nf.v)]
                connect = [] if nd.connect is None else list(nd.connect)
                if l == 0:
                    cur[:, :, k] = R.evaluate(xx[:, list(nd.input_dim) + connect], W, Omega, b, theta, v, kind, length, scale)
                    continue
                for p in range(P):
                    a = slice(p, p + 1)
                    xin = np.concatenate((vals[-1][p][:, list(nd.input_dim)], xx[:, connect]), 1)
                    cur[a, :, k] = R.evaluate(xin, W[nf.group[p]], Omega, b, theta[a], v[a], kind, length, scale)
            vals.append(cur)
        return [[cur[:, :, k].T for k in range(cur.shape[2])] for cur in vals] if container else vals[-1][:, :, 0]

    Jn = replay(pf, x, composed(x, container=True))[-1][0][:, :, 0]   # (P, M, Dx), numpy alone
    dev_numpy = np.abs(G.central(composed, x, h) - Jn).max() / np.abs(Jn).max()
    print('numpy replay: central differences against its chain rule: %.3g of max |J| (1e-7)' % dev_numpy)
    assert dev_numpy <= 1e-7
    grad = pf.grad(x)[0].transpose(2, 0, 1)   # (P, M, Dx)
    fd = G.central(lambda xx: pf(xx)[0].T, x, h)
    dev = np.abs(fd - grad).max() / np.abs(grad).max()
    print('central differences of paths(x) against paths.grad(x): %.3g of max |grad| (1e-6)' % dev)
    assert dev <= 1e-6


@pytest.mark.parametrize('which', ['hetero', 'categorical'])
def test_sampled_nodes_are_refused(eng, which):
    from dgp_amd import emulator
    X, mdl = model(which)
    emu = emulator(mdl.estimate(), N=2, seed=5)
    pf = emu.sample_functions(sample_size=2, n_features=32)
    x = np.random.default_rng(1).uniform(size=(5, X.shape[1]))
    for call in (pf.grad, pf.value_and_grad):
        with pytest.raises(ValueError, match='a sampled node has no derivative'):
            call(x)
    out = pf(x)
    assert out[0].shape[0] == 5 and np.all(np.isfinite(out[0]))


def test_bad_rows_raise_as_paths_does(eng):
    from dgp_amd import emulator
    from test_gpu_pathfun import _gp
    X, mdl = model('two-connect')
    emu = emulator(mdl.estimate(), N=2, seed=1)
    pf = emu.sample_functions(sample_size=2, n_features=16)
    rng = np.random.default_rng(2)
    Xg = rng.uniform(size=(30, 2))
    gpaths = _gp('sexp', Xg, np.sin(4 * Xg[:, :1])).sample_functions(sample_size=2, n_features=16)
    for obj, rows in ((pf, X), (gpaths, Xg)):
        for call in (obj.grad, obj.value_and_grad):
            with pytest.raises(Exception, match='2d-array'):
                call(rows[0])
            with pytest.raises(Exception, match='2d-array'):
                call(rows[None])
            with pytest.raises(ValueError, match='no rows'):
                call(rows[:0])
