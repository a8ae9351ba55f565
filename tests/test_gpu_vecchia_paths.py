"""Vecchia joint sample paths (dgpamd_vpaths_nn, dgpamd_vpaths_rows, vpaths, emulator / gp .sample_paths_vecchia).
Needs an MI355X: -m gpu.

The references restate the definition in numpy: brute-force conditioning sets in (distance, combined index) order, each
row's b_i = A^-1 a and d_i by numpy.linalg.solve, and the draw v_i = sum b_ij (y or v)_j + sqrt(d_i) z_i row by row."""
import copy
import warnings

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


def corr(kind, A, B):
    d = A[:, None, :] - B[None, :, :]
    if kind == 'sexp':
        return np.exp(-(d ** 2).sum(-1))
    r = np.abs(d)
    return np.prod(1 + np.sqrt(5) * r + 5 / 3 * r ** 2, -1) * np.exp(-np.sqrt(5) * r.sum(-1))


def brute_nn(q, x, m):
    """(M, m) combined indices of c(i) for ordered, scaled test rows q against scaled training rows x."""
    n, M = len(x), len(q)
    out = -np.ones((M, m), np.int64)
    for i in range(M):
        C = np.concatenate((x, q[:i]))
        d = ((C - q[i]) ** 2).sum(1)
        idx = np.lexsort((np.arange(len(C)), d))[:min(m, n + i)]
        out[i, :len(idx)] = idx
    return out


def row_ref(kind, q, x, nn, i, nugget, omega):
    """(members, b_i, Schur 1 + nugget - a^T b_i) of position i."""
    n = len(x)
    mem = nn[nn >= 0]
    P = np.concatenate((x, q))[mem]
    A = corr(kind, P, P)
    A[np.diag_indices(len(mem))] = 1.0 + nugget * np.where(mem < n, omega[np.minimum(mem, n - 1)], 1.0)
    a = corr(kind, P, q[i:i + 1])[:, 0]
    b = np.linalg.solve(A, a)
    return mem, b, 1.0 + nugget - a @ b


def draw_ref(kind, W, y, omega, length, scale, nugget, X, m, order, z):
    """One path of one node by the definition: X (M, D) in x's row order, z (M) indexed by x's rows."""
    n, M = len(W), len(X)
    q, xs = X[order] / length, W / length
    nn = brute_nn(q, xs, min(m, n + M - 1))
    v = np.zeros(M)
    for i in range(M):
        mem, b, s = row_ref(kind, q, xs, nn[i], i, nugget, omega)
        vals = np.where(mem < n, y[np.minimum(mem, n - 1)], v[np.maximum(mem - n, 0)])
        v[i] = b @ vals + np.sqrt(scale * s) * z[order[i]]
    out = np.empty(M)
    out[order] = v
    return out


# ------------------------------------------------------------------------------------------------ operators
@pytest.mark.parametrize('case', ['shared', 'per_path'])
@pytest.mark.parametrize('D', [1, 5, 20])
@pytest.mark.parametrize('n,m', [(40, 12), (7, 12), (30, 70)])
def test_neighbour_search_equals_brute_force(eng, case, D, n, m):
    import torch
    rng = np.random.default_rng(D * 100 + n + m)
    M, G = 33, 3
    X = rng.uniform(size=(G, n, D))
    X[1, 5 % n] = X[1, 2 % n]   # a tie
    if case == 'shared':
        Q, group = rng.uniform(size=(1, M, D)), None
    else:
        Q = rng.uniform(size=(5, M, D))
        Q[2, 9] = Q[2, 4]
        group = np.array([2, 0, 1, 1, 2], np.int32)
    g = None if group is None else torch.as_tensor(group, device=eng.device)
    out = npy(eng.vpaths_nn(eng.tensor(Q), eng.tensor(X), m, g))
    for p in range(len(Q)):
        ref = brute_nn(Q[p], X[0 if group is None else group[p]], m)
        np.testing.assert_array_equal(out[p], ref)


@pytest.mark.parametrize('form', [dict(m=20, D=3), dict(m=51, D=12), dict(m=80, D=20)])
@pytest.mark.parametrize('extra', ['plain', 'replicates'])
@pytest.mark.parametrize('kind', ['sexp', 'matern2.5'])
def test_rows_equal_numpy(eng, kind, extra, form):
    """b_i (training part through unit right-hand sides, test part from the rows), sqrt(d_i) and t_i, per path and group;
    m = 80, D = 20 takes the LDS kernel.  The two smaller forms take the register kernel, and once more the LDS kernel (an
    engine created under DGPAMD_VECCHIA_LDS=1): held to the same reference at the same tolerances, and to the register
    kernel's rows within test_vecchia_row_kernels_register_and_lds_versions_agree's bound for the same pair of designs."""
    import torch
    from test_gpu_ops import engine_under
    m, D = form['m'], form['D']
    rng = np.random.default_rng(m + D)
    n, M, P, nugget, scale = 45, 70, 3, 3e-3, 1.7
    X = rng.uniform(size=(2, n, D)) * 2
    Q = rng.uniform(size=(P, M, D)) * 2
    omega = np.ones(n) if extra == 'plain' else rng.choice([1.0, 0.5, 1 / 3], size=n)
    group = np.array([1, 0, 1], np.int32)
    Y = np.concatenate((np.eye(n)[None].repeat(2, 0), rng.normal(size=(2, 1, n))), 1)   # (G, n + 1, n)
    dNN = eng.vpaths_nn(eng.tensor(Q), eng.tensor(X), m, torch.as_tensor(group, device=eng.device))
    NN = npy(dNN)
    refs = [[row_ref(kind, Q[p], X[group[p]], NN[p, i], i, nugget, omega) for i in range(M)] for p in range(P)]

    def rows(e):
        Lr, NNl, t, sd, info = e.vpaths_rows(kind, eng.tensor(Q), eng.tensor(X), dNN, eng.tensor(Y), scale, nugget,
                                             None if extra == 'plain' else eng.tensor(omega),
                                             torch.as_tensor(group, device=eng.device))
        assert int(npy(info)[0]) == 0
        Lr, NNl, t, sd = npy(Lr), npy(NNl), npy(t), npy(sd)
        for p in range(P):
            for i in range(M):
                mem, b, s = refs[p][i]
                tol = 1e-10 * max(1.0, np.abs(b).max())
                assert abs(sd[p, i] - np.sqrt(scale * s)) <= 1e-10 * np.sqrt(scale * s)
                tr, te = mem < n, mem >= n
                np.testing.assert_allclose(t[p, mem[tr], i], b[tr], rtol=0, atol=tol)   # unit right-hand sides
                np.testing.assert_allclose(t[p, n, i], Y[group[p], n, mem[tr]] @ b[tr], rtol=0, atol=tol * np.abs(Y).max() * n)
                k = te.sum()
                assert Lr[p, i, 0] == pytest.approx(1 / sd[p, i], rel=1e-14) and NNl[p, i, 0] == i
                np.testing.assert_array_equal(NNl[p, i, 1:1 + k], mem[te] - n)
                np.testing.assert_allclose(-Lr[p, i, 1:1 + k] * sd[p, i], b[te], rtol=0, atol=tol)
                assert np.all(NNl[p, i, 1 + k:] == -1) and np.all(Lr[p, i, 1 + k:] == 0)
        return Lr, NNl, t, sd

    reg = rows(eng)
    if m <= 51:
        with engine_under(VECCHIA_LDS=1) as e:
            lds = rows(e)
        np.testing.assert_array_equal(lds[1], reg[1])
        for a, b in zip((lds[0], lds[2], lds[3]), (reg[0], reg[2], reg[3])):
            np.testing.assert_allclose(a, b, rtol=1e-9, atol=1e-9 * np.abs(b).max())


@pytest.mark.parametrize('s', [1.0, 1e4])
@pytest.mark.parametrize('kind', ['sexp', 'matern2.5'])
def test_rows_beyond_the_exponent_range(eng, kind, s):
    """Training rows i s (1, 1) against a lengthscale of 1e-5 (squared-exponential exponents 2e10 i^2 and beyond 2^63, Matern ones
    sqrt5 2e5 i and sqrt5 2e9 i: far beyond 2^31 ln 2 = 1.4886e9, where exp_negated's integer part leaves 32 bits), P = 2 paths of
    M = 16 test rows -- path 0 half on training rows and half between them, path 1 all between --, n = 64, m = 8.  Every correlation
    between different points is exactly 0 in numpy: the b_i are e_j / (1 + nugget) or 0.  test_rows_equal_numpy's tolerances; what
    is exactly 0 in the restatement may be 1e-300 here at the most."""
    import torch
    rng = np.random.default_rng(16)
    n, M, P, m, nugget, scale, length = 64, 16, 2, 8, 1e-6, 1.1, 1e-5
    X = (far_inputs(n, s) / length)[None]
    pos = np.stack([np.concatenate((rng.permutation(n)[:8], rng.permutation(n)[:8] + 0.25)), rng.permutation(n)[:M] + 0.5])
    Q = pos[:, :, None] * s * np.ones((1, 1, 2)) / length
    omega = np.ones(n)
    Y = np.concatenate((np.eye(n)[None], rng.normal(size=(1, 1, n))), 1)   # (1, n + 1, n)
    NN = eng.vpaths_nn(eng.tensor(Q), eng.tensor(X), m, None)
    Lr, NNl, t, sd, info = eng.vpaths_rows(kind, eng.tensor(Q), eng.tensor(X), NN, eng.tensor(Y), scale, nugget)
    assert int(npy(info)[0]) == 0
    Lr, NNl, t, sd, NN = npy(Lr), npy(NNl), npy(t), npy(sd), npy(NN)

    def close_or_zero(a, ref, atol):
        nz = check_zeros(a, ref)
        np.testing.assert_allclose(a[nz], ref[nz], rtol=0, atol=atol)

    hits = 0
    for p in range(P):
        for i in range(M):
            mem, b, sch = row_ref(kind, Q[p], X[0], NN[p, i], i, nugget, omega)
            hits += np.count_nonzero(b)
            tol = 1e-10 * max(1.0, np.abs(b).max())
            assert abs(sd[p, i] - np.sqrt(scale * sch)) <= 1e-10 * np.sqrt(scale * sch)
            tr, te = mem < n, mem >= n
            close_or_zero(t[p, mem[tr], i], b[tr], tol)
            np.testing.assert_allclose(t[p, n, i], Y[0, n, mem[tr]] @ b[tr], rtol=0, atol=tol * np.abs(Y).max() * n)
            k = te.sum()
            assert Lr[p, i, 0] == pytest.approx(1 / sd[p, i], rel=1e-14) and NNl[p, i, 0] == i
            np.testing.assert_array_equal(NNl[p, i, 1:1 + k], mem[te] - n)
            close_or_zero(-Lr[p, i, 1:1 + k] * sd[p, i], b[te], tol)
            assert np.all(NNl[p, i, 1 + k:] == -1) and np.all(Lr[p, i, 1 + k:] == 0)
    assert hits == 8


def test_rows_refuse_a_block_over_the_lds(eng):
    from dgp_amd.ops import DgpAmdError
    n, M, D, m = 300, 4, 64, 140
    X, Q = np.zeros((1, n, D)), np.zeros((1, M, D))
    NN = eng.vpaths_nn(eng.tensor(Q), eng.tensor(X), m)
    with pytest.raises(DgpAmdError, match='LDS'):
        eng.vpaths_rows('sexp', eng.tensor(Q), eng.tensor(X), NN, eng.tensor(np.zeros((1, 1, n))), 1.0, 1e-3)


# ------------------------------------------------------------------------------------------------ exactness
def dense_joint(kind, W, y, omega, length, scale, nugget, X):
    n = len(W)
    R = corr(kind, W / length, W / length) + nugget * np.diag(omega)
    Ks = corr(kind, W / length, X / length)
    Kss = corr(kind, X / length, X / length) + nugget * np.eye(len(X))
    mean = Ks.T @ np.linalg.solve(R, y)
    return mean, scale * (Kss - Ks.T @ np.linalg.solve(R, Ks))


@pytest.mark.parametrize('n,M,m', [(30, 20, 49), (60, 40, 99)])
@pytest.mark.parametrize('kind', ['sexp', 'matern2.5'])
def test_full_conditioning_sets_give_the_dense_joint(eng, kind, n, M, m):
    from dgp_amd import vpaths
    from dgp_amd.paths import factor_inverse
    rng = np.random.default_rng(n + M)
    D, scale, nugget, length = 2, 1.3, 1e-2, np.array([0.5, 0.7])
    W, X = rng.uniform(size=(n, D)), rng.uniform(size=(M, D))
    y = np.sin(3 * W[:, 0]) + W[:, 1]
    omega = np.ones(n)
    order = rng.permutation(M)
    Z = np.concatenate((np.zeros((1, M)), np.eye(M)))
    V = npy(vpaths.Vecchia(m, order).draw_shared(eng, (kind, length, scale, nugget), eng.tensor(X), (eng.tensor(W), None),
                                                 eng.tensor(y[None]), eng.tensor(Z), M + 1))
    mean, Sig = dense_joint(kind, W, y, omega, length, scale, nugget, X)
    np.testing.assert_allclose(V[0], mean, rtol=0, atol=1e-9 * max(1.0, np.abs(mean).max()))
    F = (V[1:] - V[0]).T
    np.testing.assert_allclose(F @ F.T, Sig, rtol=0, atol=1e-9 * scale)
    Li = factor_inverse(eng, kind, eng.tensor(W), None, None, length, nugget, 'test')
    A, _ = eng.joint_cov(kind, eng.tensor(X), eng.tensor(W), Li, eng.tensor(y[None]), length, scale, nugget)
    low = np.tril(np.ones((M, M), bool))
    np.testing.assert_allclose((F @ F.T)[low], npy(A[0])[:M, :M][low], rtol=0, atol=1e-9 * scale)


def test_first_row_agrees_with_vecchia_predict(eng):
    import torch
    from dgp_amd import gp, kernel, vpaths
    rng = np.random.default_rng(4)
    X = rng.uniform(size=(300, 3))
    Y = (np.sin(4 * X[:, 0]) + X[:, 1] * X[:, 2])[:, None]
    for kind in ('sexp', 'matern2.5'):
        mdl = gp(X, Y, kernel(length=np.array([0.4, 0.6, 0.5]), name=kind, scale=1.4, nugget=1e-3), vecchia=True, m=20)
        x = rng.uniform(size=(50, 3))
        mu, s2 = mdl.predict(x, m=30)
        k = mdl.kernel
        order = rng.permutation(50)
        V = npy(vpaths.Vecchia(30, order).draw_shared(eng, (kind, k.length, k.scale[0], k.nugget[0]), eng.tensor(x),
                                                      (eng.tensor(k._X()), None), eng.tensor(k.output.reshape(1, -1)),
                                                      torch.zeros(1, 50, dtype=torch.float64, device=eng.device), 1))
        r0 = order[0]
        assert abs(V[0, r0] - mu[r0, 0]) <= 1e-10 * max(1.0, abs(mu[r0, 0]))
        q = eng.tensor(x[order][None] / k.length)
        xs = eng.tensor(k._X()[None] / k.length)
        NN = eng.vpaths_nn(q, xs, 30)
        _, _, _, sd, _ = eng.vpaths_rows(kind, q, xs, NN, eng.tensor(k.output.reshape(1, 1, -1)), k.scale[0], k.nugget[0])
        assert abs(npy(sd)[0, 0] ** 2 - s2[r0, 0]) <= 1e-10 * s2[r0, 0]


# ------------------------------------------------------------------------------------------------ models
def _two_layer(kind, n=80, seed=0):
    from dgp_amd import dgp, kernel, combine
    rng = np.random.default_rng(seed)
    X = rng.uniform(size=(n, 2))
    Y = (np.sin(5 * X[:, :1]) * np.cos(3 * X[:, 1:]) + 0.02 * rng.normal(size=(n, 1)))
    layers = combine([kernel(length=np.array([0.8]), name=kind, nugget=1e-4) for _ in range(2)],
                     [kernel(length=np.array([1.0]), name=kind, scale_est=True, nugget=1e-4, connect=np.arange(2))])
    model = dgp(X, Y, layers, seed=seed)
    model.train(N=3, ess_burn=3, disable=True)
    return X, model


def _walk_reference(emu, x, J, m, rng):
    S, M = emu.N, len(x)
    order = rng.permutation(M)
    outs, prev = [], None
    for l, layer in enumerate(emu.all_layer):
        cur = np.empty((S * J, M, len(layer)))
        for k, nd in enumerate(layer):
            Z = rng.standard_normal((S, J, M))
            gl = None if nd.connect is None else x[:, nd.connect]
            omega = np.ones(len(nd.output)) if nd.rep is None else nd.W_diag
            for s in range(S):
                y = emu.latents[s][l][:, k] if l < emu.n_layer - 1 else np.asarray(nd.output, float).reshape(-1)
                if l == 0:
                    W = nd._X()
                else:
                    W = emu.latents[s][l - 1][:, nd.input_dim]
                    if nd.connect is not None:
                        W = np.concatenate((W, nd.global_input), 1)
                for j in range(J):
                    p = s * J + j
                    xin = x[:, nd.input_dim] if l == 0 else prev[p][:, nd.input_dim]
                    if gl is not None:
                        xin = np.concatenate((xin, gl), 1)
                    cur[p, :, k] = draw_ref(nd.name, W, y, omega, nd.length, nd.scale[0], nd.nugget[0], xin, m, order,
                                            Z[s, j])
        outs.append(cur)
        prev = cur
    return outs


@pytest.mark.parametrize('mode', ['dense', 'vecchia'])
@pytest.mark.parametrize('kind', ['sexp', 'matern2.5'])
def test_emulator_paths_replay_the_definition(eng, kind, mode):
    from dgp_amd import emulator
    _, model = _two_layer(kind)
    emu = emulator(model.estimate(), N=2, seed=5)
    if mode == 'vecchia':
        emu.to_vecchia()
    x = np.random.default_rng(8).uniform(size=(30, 2))
    rng = copy.deepcopy(emu._sample_rng)
    out = emu.sample_paths_vecchia(x, sample_size=3, full_layer=True, m=12)
    ref = _walk_reference(emu, x, 3, 12, rng)
    assert len(out) == 2 and len(out[0]) == 2 and len(out[1]) == 1
    for l in range(2):
        for k in range(len(out[l])):
            assert out[l][k].shape == (30, 6)
            np.testing.assert_allclose(out[l][k], ref[l][:, :, k].T, rtol=1e-8, atol=1e-8)


@pytest.mark.parametrize('kind', ['sexp', 'matern2.5'])
def test_gp_paths_replay_the_global_generator(eng, kind):
    from dgp_amd import gp, kernel
    rng = np.random.default_rng(11)
    X = rng.uniform(size=(60, 3))
    X = np.concatenate((X, X[:10]))
    Y = (np.sin(3 * X[:, 0]) + X[:, 1] * X[:, 2] + 0.05 * rng.normal(size=len(X)))[:, None]
    mdl = gp(X, Y, kernel(length=np.full(3, 0.7), name=kind, scale=1.9, nugget=1e-3, input_dim=np.array([0, 1]),
                          connect=np.array([2])))
    xt = rng.uniform(size=(35, 3))
    np.random.seed(21)
    out = mdl.sample_paths_vecchia(xt, sample_size=4, m=15)
    assert out.shape == (35, 4)
    np.random.seed(21)
    order = np.random.permutation(35)
    Z = np.random.standard_normal((4, 35))
    k = mdl.kernel
    xin = np.concatenate((xt[:, [0, 1]], xt[:, [2]]), 1)
    for j in range(4):
        ref = draw_ref(kind, k._X(), k.output.reshape(-1), k.W_diag, k.length, k.scale[0], k.nugget[0], xin, 15, order, Z[j])
        np.testing.assert_allclose(out[:, j], ref, rtol=1e-8, atol=1e-8)


def test_large_m_and_monte_carlo_moments(eng):
    from dgp_amd import emulator
    _, model = _two_layer('matern2.5', n=80, seed=3)
    emu = emulator(model.estimate(), N=4, seed=7)
    emu.to_vecchia()
    rng = np.random.default_rng(12)
    big = rng.uniform(size=(20000, 2))
    out = emu.sample_paths_vecchia(big, sample_size=2)[0]
    assert out.shape == (20000, 8) and np.all(np.isfinite(out))
    x = rng.uniform(size=(20, 2))
    mu, var = emu.predict(x, m=50)
    draws = emu.sample_paths_vecchia(x, sample_size=100, m=50)[0]   # (20, 400)
    P = draws.shape[1]
    assert np.all(np.abs(draws.mean(1) - mu[:, 0]) <= 5 * np.sqrt(var[:, 0] / P))


@pytest.mark.parametrize('top', ['Poisson', 'Categorical'])
def test_likelihood_tops(eng, top):
    from dgp_amd import dgp, kernel, combine, emulator, Poisson, Categorical
    rng = np.random.default_rng(6)
    n = 50
    X = rng.uniform(size=(n, 2))
    K = lambda **kw: kernel(length=np.array([1.0]), name='matern2.5', nugget=1e-4, **kw)
    if top == 'Poisson':
        Y = rng.poisson(np.exp(1 + np.sin(4 * X[:, [0]]))).astype(float)
        layers = combine([K() for _ in range(2)], [K(scale_est=True)], [Poisson()])
    else:
        Y = (X[:, [0]] + 0.3 * np.sin(6 * X[:, [1]]) > 0.55).astype(int)
        layers = combine([K() for _ in range(2)], [K(scale_est=True)], [Categorical(num_classes=2)])
    model = dgp(X, Y, layers, seed=4)
    model.train(N=3, ess_burn=3, disable=True)
    emu = emulator(model.estimate(), N=2, seed=2)
    x = rng.uniform(size=(30, 2))
    np.random.seed(3)
    dense = emu.sample_paths(x, sample_size=5, full_layer=True)
    np.random.seed(3)
    vec = emu.sample_paths_vecchia(x, sample_size=5, full_layer=True, m=20)
    assert [len(f) for f in vec] == [len(f) for f in dense]
    for fv, fd in zip(vec, dense):
        for a, b in zip(fv, fd):
            assert a.shape == b.shape and a.dtype == b.dtype
    last = vec[-1][0]
    if top == 'Poisson':
        assert np.all(last >= 0) and np.all(last == np.round(last))
    else:
        assert np.all((last >= 0) & (last <= 1))


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(eng):
    import torch
    from dgp_amd import emulator, gp, kernel
    rng = np.random.default_rng(2)
    X = rng.uniform(size=(40, 2))
    Y = np.sin(4 * X[:, :1])
    _, model = _two_layer('sexp', n=60)
    emu = emulator(model.estimate(), N=2, seed=1)
    dg = gp(X, Y, kernel(length=np.array([0.5]), name='sexp'))
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    emu.shard = True
    with pytest.raises(NotImplementedError):
        emu.sample_paths_vecchia(X[:5])
    emu.shard = False
    with pytest.raises(Exception, match='2d-array'):
        emu.sample_paths_vecchia(X[:5, 0])
    with pytest.raises(ValueError):
        emu.sample_paths_vecchia(X[:5], m=0)
    with pytest.raises(Exception, match='2d-array'):
        dg.sample_paths_vecchia(X[:5, 0])
    with pytest.raises(ValueError):
        dg.sample_paths_vecchia(X[:5], m=0)
    assert torch.cuda.memory_allocated() == before


def test_a_test_point_on_a_training_point_without_nugget(eng):
    from dgp_amd import gp, kernel
    rng = np.random.default_rng(9)
    X = rng.uniform(size=(40, 2))
    Y = np.sin(4 * X[:, :1]) + X[:, 1:]
    mdl = gp(X, Y, kernel(length=np.array([0.6, 0.9]), name='matern2.5', nugget=0.0, scale=1.7, nugget_est=False))
    xt = np.concatenate((X[[3]], rng.uniform(size=(5, 2))))
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        try:
            out = mdl.sample_paths_vecchia(xt, sample_size=3, m=10)
            assert np.all(np.isfinite(out))
            assert any('did not factor' in str(w.message) and 'the gp model' in str(w.message) for w in rec)
        except np.linalg.LinAlgError as err:
            assert 'the gp model' in str(err)
