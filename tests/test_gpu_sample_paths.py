"""Joint posterior sample paths (dgpamd_joint_cov, dgpamd_mvn_paths, gp.sample_paths, emulator.sample_paths).  Needs an
MI355X: -m gpu.

The numpy references take a different route from the device: the Cholesky factor of the joint (n + M) matrix
[[R, K*], [K*^T, K** + nugget I]].  Its blocks give mean = L21 (L11^-1 y) and Sigma = scale L22 L22^T, and one path is
mean + sqrt(scale) L22 e.  No inverse is formed anywhere."""
import copy

import numpy as np
import pytest

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


def close(a, b, rtol, atol):
    np.testing.assert_allclose(np.asarray(a, float), np.asarray(b, float), rtol=rtol, atol=atol)


def joint_ref(W, x, y, length, nugget, kind, wdiag=None):
    """(mean (M, r), L22) of the posterior at x by the joint Cholesky; y: (r, n)."""
    from oracle import dgp_oracle as O
    n = len(W)
    R = O.corr_matrix(W, length, kind)
    R[np.arange(n), np.arange(n)] = 1.0 + nugget * (1.0 if wdiag is None else wdiag)
    Ks = O.cross_corr(W, x, length, kind)
    Kss = O.corr_matrix(x, length, kind)
    Kss[np.arange(len(x)), np.arange(len(x))] = 1.0 + nugget
    C = np.block([[R, Ks], [Ks.T, Kss]])
    Lj = np.linalg.cholesky(C)
    L11, L21, L22 = Lj[:n, :n], Lj[n:, :n], Lj[n:, n:]
    w = np.linalg.solve(L11, np.atleast_2d(y).T)
    return L21 @ w, L22


def ref_path(W, x, y, length, nugget, scale, kind, eps, wdiag=None):
    mean, L22 = joint_ref(W, x, y, length, nugget, kind, wdiag)
    return mean[:, 0] + np.sqrt(scale) * L22 @ eps


def linv(eng, kind, W, length, nugget):
    from dgp_amd import paths
    return paths.factor_inverse(eng, kind, eng.tensor(W), None, None, length, nugget, 'test')


# ------------------------------------------------------------------------------------------------ operator
@pytest.mark.parametrize('M', [1, 64, 65, 130, 2100])
@pytest.mark.parametrize('n', [1, 63, 64, 65, 200])
@pytest.mark.parametrize('nlen', ['one', 'D'])
@pytest.mark.parametrize('kind', ['sexp', 'matern2.5'])
def test_joint_cov_matches_the_joint_cholesky(eng, kind, nlen, n, M):
    rng = np.random.default_rng(n * 7 + M)
    D, scale, nugget = 3, 1.7, 1e-3
    length = np.array([0.8]) if nlen == 'one' else np.array([0.6, 1.1, 0.9])
    W, x = rng.uniform(size=(n, D)), rng.uniform(size=(M, D))
    y = rng.normal(size=(2, n))
    Li = linv(eng, kind, W, length, nugget)
    A, mean = eng.joint_cov(kind, eng.tensor(x), eng.tensor(W), Li, eng.tensor(y), length, scale, nugget)
    mref, L22 = joint_ref(W, x, y, length, nugget, kind)
    S = npy(A[0])
    Mp = eng.padded_dim(M)
    assert S.shape == (Mp, Mp)
    low = np.tril(np.ones((M, M), bool))
    close(S[:M, :M][low], (scale * L22 @ L22.T)[low], rtol=0, atol=1e-10 * scale)
    close(npy(mean[0]), mref, rtol=0, atol=1e-10 * scale * max(1.0, np.abs(mref).max()))
    # the padding the factorisation expects: zero outside [0, M)^2 in the lower tiles
    tiles = np.kron(np.tril(np.ones((Mp // 64, Mp // 64))), np.ones((64, 64))).astype(bool)
    pad = tiles.copy()
    pad[:M, :M] = False
    assert np.all(S[pad] == 0.0)
    # diag(Sigma) and mean are dgpamd_gp_predict's variance and mean -- up to the rounding of its R^-1 form, whose terms
    # reach |R^-1| ~ 1/nugget and cancel: bounded per point by n eps sum_ij |r_i| |R^-1_ij| |r_j| (and the same with y)
    from oracle import dgp_oracle as O
    R = O.corr_matrix(W, length, kind) + nugget * np.eye(n)
    Rinv = np.linalg.inv(R)
    mu, var = eng.gp_predict(kind, eng.tensor(x), eng.tensor(W), length, eng.tensor(Rinv), n, eng.tensor(y @ Rinv),
                             scale, nugget)
    r = np.abs(O.cross_corr(W, x, length, kind))
    eps = np.finfo(float).eps
    tol_v = 1e-9 * scale + scale * n * eps * np.einsum('it,ij,jt->t', r, np.abs(Rinv), r)
    assert np.all(np.abs(np.diag(S)[:M] - npy(var)) <= tol_v)
    tol_m = 1e-9 * scale * max(1.0, np.abs(mref).max()) + n * eps * (np.abs(y) @ np.abs(Rinv) @ r)
    assert np.all(np.abs(npy(mean[0]).T - npy(mu)) <= tol_m)


@pytest.mark.parametrize('kind', ['sexp', 'matern2.5'])
def test_joint_cov_batches_items_over_groups(eng, kind):
    """Three items sharing one group (one pack of the L^-1 tiles), then five items over two groups in the order
    0, 1, 1, 0, 1: every item as its own single call."""
    import torch
    rng = np.random.default_rng(3)
    D, n, M, scale, nugget = 2, 150, 70, 0.6, 1e-3
    length = np.array([0.5, 0.7])
    W = [rng.uniform(size=(n, D)) for _ in range(2)]
    y = [rng.normal(size=(1, n)) for _ in range(2)]
    Li = torch.stack([linv(eng, kind, W[g], length, nugget) for g in range(2)]).contiguous()
    Wd, yd = eng.tensor(np.stack(W)), eng.tensor(np.stack(y))
    for group in ([0, 0, 0], [0, 1, 1, 0, 1]):
        x = rng.uniform(size=(len(group), M, D))
        A, mean = eng.joint_cov(kind, eng.tensor(x), Wd, Li, yd, length, scale, nugget, group=group)
        for b, g in enumerate(group):
            mref, L22 = joint_ref(W[g], x[b], y[g], length, nugget, kind)
            close(np.tril(npy(A[b])[:M, :M]), np.tril(scale * L22 @ L22.T), rtol=0, atol=1e-10 * scale)
            close(npy(mean[b]), mref, rtol=0, atol=1e-10 * max(1.0, np.abs(mref).max()))


@pytest.mark.parametrize('kind', ['sexp', 'matern2.5'])
def test_joint_cov_at_64_inputs(eng, kind):
    rng = np.random.default_rng(64)
    D, n, M, scale, nugget = 64, 130, 90, 1.3, 1e-2
    length = np.sqrt(D) * rng.uniform(0.8, 1.2, size=D)
    W, x, y = rng.uniform(size=(n, D)), rng.uniform(size=(M, D)), rng.normal(size=(3, n))
    A, mean = eng.joint_cov(kind, eng.tensor(x), eng.tensor(W), linv(eng, kind, W, length, nugget), eng.tensor(y), length,
                            scale, nugget)
    mref, L22 = joint_ref(W, x, y, length, nugget, kind)
    close(np.tril(npy(A[0])[:M, :M]), np.tril(scale * L22 @ L22.T), rtol=0, atol=1e-10 * scale)
    close(npy(mean[0]), mref, rtol=0, atol=1e-10 * max(1.0, np.abs(mref).max()))


@pytest.mark.parametrize('c', [1, 5, 40])
def test_mvn_paths_is_mean_plus_factor_times_normals(eng, c):
    rng = np.random.default_rng(c)
    M, B, rep = 130, 2, (5 if c > 1 else 1)
    G = rng.normal(size=(B, M, M))
    S = G @ G.transpose(0, 2, 1) / M + np.eye(M)
    Mp = eng.padded_dim(M)
    A = np.zeros((B, Mp, Mp))
    A[:, :M, :M] = np.tril(S)
    Ad = eng.tensor(A)
    _, info = eng.potrf(M, Ad, batch=B)
    assert not npy(info).any()
    E, mean = rng.normal(size=(B, M, c)), rng.normal(size=(B, M, c // rep))
    out = npy(eng.mvn_paths(Ad, eng.tensor(mean), eng.tensor(E), rep=rep))
    for b in range(B):
        L = np.linalg.cholesky(S[b])
        close(out[b], np.repeat(mean[b], rep, axis=1) + L @ E[b], rtol=1e-12, atol=1e-11)


# ------------------------------------------------------------------------------------------------ gp
def _gp(kind, X, Y, connect=None, nugget=1e-4):
    from dgp_amd import gp, kernel
    D = X.shape[1]
    k = kernel(length=np.full(D, 0.7), name=kind, scale=1.9, nugget=nugget,
               input_dim=None if connect is None else np.setdiff1d(np.arange(D), connect), connect=connect)
    return gp(X, Y, k)


@pytest.mark.parametrize('case', ['plain', 'connect', 'replicates'])
@pytest.mark.parametrize('kind', ['sexp', 'matern2.5'])
def test_gp_sample_paths_replays_numpy(eng, kind, case):
    rng = np.random.default_rng(11)
    X = rng.uniform(size=(60, 3))
    if case == 'replicates':
        X = np.concatenate((X, X[:15]))
    Y = (np.sin(3 * X[:, 0]) + X[:, 1] * X[:, 2] + 0.05 * rng.normal(size=len(X)))[:, None]
    m = _gp(kind, X, Y, connect=np.array([2]) if case == 'connect' else None)
    xt = rng.uniform(size=(35, 3))
    np.random.seed(21)
    out = m.sample_paths(xt, sample_size=7)
    assert out.shape == (35, 7)
    np.random.seed(21)
    Z = np.random.standard_normal((7, 35))
    k = m.kernel
    cols = np.concatenate((np.setdiff1d(np.arange(3), [2]), [2])) if case == 'connect' else np.arange(3)
    W = k._X()
    mean, L22 = joint_ref(W, xt[:, cols], np.asarray(k.output).reshape(1, -1), k.length, k.nugget[0], kind,
                          None if k.rep is None else k.W_diag)
    ref = mean + np.sqrt(k.scale[0]) * L22 @ Z.T
    close(out, ref, rtol=1e-7, atol=1e-7 * np.sqrt(k.scale[0]))


# ------------------------------------------------------------------------------------------------ emulator
def _two_layer(kind, n=100, seed=0):
    from dgp_amd import dgp, kernel, combine
    rng = np.random.default_rng(seed)
    X = rng.uniform(size=(n, 2))
    Y = (np.sin(5 * X[:, :1]) * np.cos(3 * X[:, 1:]) + 0.02 * rng.normal(size=(n, 1)))
    layers = combine([kernel(length=np.array([0.8]), name=kind, nugget=1e-4) for _ in range(2)],
                     [kernel(length=np.array([1.0]), name=kind, scale_est=True, nugget=1e-4, connect=np.arange(2))])
    model = dgp(X, Y, layers, seed=seed)
    model.train(N=3, ess_burn=3, disable=True)
    return X, model


def _walk_reference(emu, x, sample_size, Z):
    """Every path of every layer by the joint Cholesky.  Z[(l, k)]: the (N, J, M) normals of GP node k of layer l."""
    S, J, M = emu.N, sample_size, len(x)
    outs = []
    prev = None
    for l, layer in enumerate(emu.all_layer):
        cur = np.empty((S * J, M, len(layer)))
        for k, nd in enumerate(layer):
            gl = None if nd.connect is None else x[:, nd.connect]
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
                    cur[p, :, k] = ref_path(W, xin, y, nd.length, nd.nugget[0], nd.scale[0], nd.name, Z[(l, k)][s, j])
        outs.append(cur)
        prev = cur
    return outs


@pytest.mark.parametrize('kind', ['sexp', 'matern2.5'])
def test_emulator_sample_paths_replays_the_layer_walk(eng, kind):
    from dgp_amd import emulator
    _, model = _two_layer(kind)
    emu = emulator(model.estimate(), N=3, seed=5)
    x = np.random.default_rng(8).uniform(size=(40, 2))
    rng = copy.deepcopy(emu._sample_rng)
    out = emu.sample_paths(x, sample_size=4, full_layer=True)
    Z = {}
    for l, layer in enumerate(emu.all_layer):
        for k, nd in enumerate(layer):
            Z[(l, k)] = rng.standard_normal((3, 4, 40))
    ref = _walk_reference(emu, x, 4, Z)
    assert len(out) == 2 and len(out[0]) == 2 and len(out[1]) == 1
    for l in range(2):
        for k in range(len(out[l])):
            assert out[l][k].shape == (40, 12)
            close(out[l][k], ref[l][:, :, k].T, rtol=1e-6, atol=1e-6)


def test_emulator_paths_match_the_linked_moments_by_monte_carlo(eng):
    """One hidden layer: the linked-GP moments are the exact mean and variance of the propagated paths, so over ~4000
    paths (after the mixture over the imputations) the sample mean and variance at every point match
    predict(method='mean_var')."""
    from dgp_amd import emulator
    _, model = _two_layer('matern2.5', n=80, seed=3)
    emu = emulator(model.estimate(), N=4, seed=7)
    x = np.random.default_rng(12).uniform(size=(25, 2))
    mu, var = emu.predict(x)
    draws = emu.sample_paths(x, sample_size=1000)[0]   # (25, 4000)
    P = draws.shape[1]
    m_hat, v_hat = draws.mean(1), draws.var(1, ddof=1)
    assert np.all(np.abs(m_hat - mu[:, 0]) <= 5 * np.sqrt(var[:, 0] / P))
    # chi-square bound of the same confidence (normal approximation of chi2_{P-1} / (P-1), widened for the mixture's tails)
    assert np.all(np.abs(v_hat / var[:, 0] - 1) <= 6 * np.sqrt(2.0 / (P - 1)))


@pytest.mark.parametrize('top', ['Poisson', 'Categorical'])
def test_three_layers_with_a_likelihood_on_top(eng, top):
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
    state = copy.deepcopy(emu._sample_rng)
    np.random.seed(3)
    full = emu.sample_paths(x, sample_size=5, full_layer=True)
    assert [len(f) for f in full] == [2, 1, 1] and all(a.shape == (30, 10) for f in full for a in f)
    last = full[-1][0]
    if top == 'Poisson':
        assert np.all(last >= 0) and np.all(last == np.round(last))
    else:
        assert np.all((last >= 0) & (last <= 1))
        from scipy.special import expit
        close(last, expit(full[1][0]), rtol=1e-14, atol=0)   # class probabilities of this call's latent paths
    emu._sample_rng = state
    np.random.seed(3)
    short = emu.sample_paths(x, sample_size=5)
    assert len(short) == 1
    close(short[0], last, rtol=0, atol=0)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(eng):
    import torch
    from dgp_amd import emulator, gp, kernel
    from dgp_amd.paths import MAX_POINTS
    rng = np.random.default_rng(2)
    X = rng.uniform(size=(40, 2))
    Y = np.sin(4 * X[:, :1])
    vg = gp(X, Y, kernel(length=np.array([0.5]), name='sexp'), vecchia=True, m=10)
    with pytest.raises(NotImplementedError):
        vg.sample_paths(X[:5])
    _, model = _two_layer('sexp', n=60)
    emu = emulator(model.estimate(), N=2, seed=1)
    emu.to_vecchia()
    with pytest.raises(NotImplementedError):
        emu.sample_paths(X[:5])
    emu.remove_vecchia()
    emu.shard = True
    with pytest.raises(NotImplementedError):
        emu.sample_paths(X[:5])
    emu.shard = False
    before = torch.cuda.memory_allocated()
    with pytest.raises(ValueError):
        emu.sample_paths(rng.uniform(size=(MAX_POINTS + 1, 2)))
    assert torch.cuda.memory_allocated() == before
    dg = gp(X, Y, kernel(length=np.array([0.5]), name='sexp'))
    with pytest.raises(ValueError):
        dg.sample_paths(rng.uniform(size=(MAX_POINTS + 1, 2)))


def test_indefinite_training_matrix_raises(eng):
    """The indefinite R of the pseudo-inverse fallback test (a repeated input row and a slightly negative nugget):
    predict() takes pinvh there; a joint draw refuses, naming where."""
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
        emu.sample_paths(rng.uniform(size=(9, 2)), sample_size=3)
