"""Vecchia joint sample paths of linked systems (lgp.sample_paths_vecchia).  Needs an MI355X: -m gpu.

The replays walk every path of the system in numpy (test_gpu_lgp_paths._walk, its per-node draw swapped for the definition
of test_gpu_vecchia_paths.draw_ref) with the same permutation and normals.  The numpy walk asserts at every row it draws
that the conditioning set is decided by more than rounding: the m-th and (m+1)-th candidate distances differ by more than
1e-9 relative (a condition on the seeds, never a skipped comparison)."""
import copy
import warnings

import numpy as np
import pytest

import test_gpu_lgp_paths as dense_walk
from test_gpu_lgp_paths import _chain, _walk
from test_gpu_sample_paths import _gp, close
from test_gpu_vecchia_paths import draw_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    from dgp_amd.ops import Engine
    return Engine(0)


def _assert_sets_are_decided(nd, xin, m, order):
    n, M = len(nd._X()), len(xin)
    q, xs = xin[order] / nd.length, nd._X() / nd.length
    mm = min(m, n + M - 1)
    for i in range(M):
        if n + i <= mm:
            continue
        d = np.sort(((np.concatenate((xs, q[:i])) - q[i]) ** 2).sum(1))
        assert d[mm] - d[mm - 1] > 1e-9 * d[mm], 'row %d: candidates %d and %d are equidistant to rounding' % (i, mm, mm + 1)


def _vecchia_node_path(m, order):
    def node_path(nd, xin, eps):
        _assert_sets_are_decided(nd, xin, m, order)
        omega = np.ones(len(nd.output)) if nd.rep is None else nd.W_diag
        return draw_ref(nd.name, nd._X(), np.asarray(nd.output, float).reshape(-1), omega, nd.length, nd.scale[0],
                        nd.nugget[0], xin, m, order, eps)
    return node_path


def _order_and_normals(sysm, M, J, seed):
    """The contract: permutation(M) first, then one (S, J, M) block per GP node in walk order, grouped by layer."""
    np.random.seed(seed)
    order = np.random.permutation(M)
    S = len(sysm.all_layer_set)
    Z = []
    for layer in sysm.all_layer:
        zl = []
        for c in layer:
            nodes = [c.structure] if c.type == 'gp' else [nd for lay in c.structure for nd in lay]
            zl += [np.random.standard_normal((S, J, M)) for nd in nodes if nd.type == 'gp']
        Z.append(zl)
    return order, Z


def _replay(monkeypatch, sysm, x, J, m, seed, tol):
    """sample_paths_vecchia(full_layer=True) against the numpy walk, every layer and emulator; returns the device result."""
    M = len(x[0])
    order, Z = _order_and_normals(sysm, M, J, seed)
    np.random.seed(seed)
    out = sysm.sample_paths_vecchia(x, sample_size=J, full_layer=True, m=m)
    monkeypatch.setattr(dense_walk, '_node_path', _vecchia_node_path(m, order))
    ref = _walk(sysm, x, J, Z)
    S = len(sysm.all_layer_set)
    assert len(out) == len(ref) and [len(o) for o in out] == [len(r) for r in ref]
    worst = 0.0
    for l in range(len(ref)):
        for k in range(len(ref[l])):
            assert out[l][k].shape == ref[l][k].shape == (ref[l][k].shape[0], M, S * J)
            worst = max(worst, float(np.max(np.abs(out[l][k] - ref[l][k]) / (1 + np.abs(ref[l][k])))))
    print('max |device - numpy| / (1 + |numpy|): %.3e (bound %g)' % (worst, tol))
    for l in range(len(ref)):
        for k in range(len(ref[l])):
            close(out[l][k], ref[l][k], rtol=tol, atol=tol)
    return out


# ------------------------------------------------------------------------------------------------ one GP container
@pytest.mark.parametrize('mode', ['dense', 'vecchia'])
@pytest.mark.parametrize('case', ['plain', 'connect', 'replicates'])
@pytest.mark.parametrize('kind', ['sexp', 'matern2.5'])
def test_one_gp_container_equals_gp_sample_paths_vecchia(eng, kind, case, mode):
    from dgp_amd.linkgp import container, lgp
    rng = np.random.default_rng(11)
    X = rng.uniform(size=(60, 3))
    if case == 'replicates':
        X = np.concatenate((X, X[:15]))
    Y = (np.sin(3 * X[:, 0]) + X[:, 1] * X[:, 2] + 0.05 * rng.normal(size=len(X)))[:, None]
    mdl = _gp(kind, X, Y, connect=np.array([2]) if case == 'connect' else None)
    sysm = lgp([[container(mdl.export(), local_input_idx=np.array([0, 1, 2]))]])
    if mode == 'vecchia':
        sysm.set_vecchia(True)
    assert len(sysm.all_layer_set) == 1
    xt = rng.uniform(size=(35, 3))
    np.random.seed(21)
    ref = mdl.sample_paths_vecchia(xt, sample_size=7, m=15)
    np.random.seed(21)
    out = sysm.sample_paths_vecchia(xt, sample_size=7, m=15)
    assert len(out) == 1 and out[0].shape == (1, 35, 7)
    close(out[0][0], ref, rtol=1e-12, atol=1e-12 * np.sqrt(mdl.kernel.scale[0]))


# ------------------------------------------------------------------------------------------------ replays of the walk
@pytest.mark.parametrize('tag', ['sexp', 'matern'])
def test_linked_chain_replays_the_walk(eng, golden, monkeypatch, tag):
    sysm, xin = _chain(eng, golden, tag)
    out = _replay(monkeypatch, sysm, xin, 3, 12, 4, 1e-6)
    assert len(out) == 3 and all(len(o) == 1 for o in out)
    np.random.seed(4)
    short = sysm.sample_paths_vecchia(xin, sample_size=3, m=12)
    assert len(short) == 1
    close(short[0], out[-1][0], rtol=0, atol=0)


def _skip_system(rng):
    """Layer 1: A (x column 0) and B (x column 1); layer 2: C on both; layer 3: D on B (layer 1, skipping layer 2) and C,
    with an external input."""
    from dgp_amd.linkgp import container, lgp
    gA = _gp('sexp', rng.uniform(size=(30, 1)), rng.normal(size=(30, 1)))
    gB = _gp('matern2.5', rng.uniform(size=(30, 1)), rng.normal(size=(30, 1)))
    gC = _gp('matern2.5', rng.normal(size=(35, 2)), rng.normal(size=(35, 1)))
    gD = _gp('sexp', rng.normal(size=(40, 3)), rng.normal(size=(40, 1)), connect=np.array([2]))
    return lgp([[container(gA.export(), local_input_idx=np.array([0])), container(gB.export(), local_input_idx=np.array([1]))],
                [container(gC.export(), local_input_idx=np.array([0, 1]))],
                [container(gD.export(), local_input_idx=[np.array([1]), np.array([0])])]])


def test_two_emulators_feeding_a_third_with_a_skip(eng, monkeypatch):
    rng = np.random.default_rng(7)
    sysm = _skip_system(rng)
    M, J = 20, 4
    x = [rng.uniform(size=(M, 2)), [None], [rng.uniform(size=(M, 1))]]
    out = _replay(monkeypatch, sysm, x, J, 12, 9, 1e-8)
    assert [len(o) for o in out] == [2, 1, 1] and all(a.shape == (1, M, J) for o in out for a in o)


def test_systems_that_cannot_share_a_call_are_split_and_scattered_back(eng, monkeypatch):
    """Three systems built by hand, GP -> GP: the second layer's node of system 2 has its own lengths and training-set
    size (a call of its own), systems 1 and 3 share kernel and shape but not the training rows (one call, two groups); the
    first layer's node of system 3 has its own outputs (one shared-input call, its y a further row of Y)."""
    from dgp_amd.linkgp import container, lgp
    rng = np.random.default_rng(13)
    X1 = rng.uniform(size=(30, 2))
    y1 = np.sin(4 * X1[:, :1]) + X1[:, 1:]
    firsts = [_gp('matern2.5', X1, y1), _gp('matern2.5', X1, y1), _gp('matern2.5', X1, y1 + 0.3 * rng.normal(size=(30, 1)))]
    seconds = []
    for s, n in enumerate((35, 28, 35)):
        W = rng.uniform(-1.5, 2.5, size=(n, 1))
        g = _gp('sexp', W, np.cos(2 * W) + 0.1 * s)
        if s == 1:
            g.kernel.length = np.array([0.45])
        seconds.append(g)
    sets = [[[container(a.export(), local_input_idx=np.array([0, 1]))], [container(b.export(), local_input_idx=np.array([0]))]]
            for a, b in zip(firsts, seconds)]
    sysm = lgp.__new__(lgp)
    sysm.L, sysm.all_layer, sysm.num_model, sysm.all_layer_set = 2, sets[0], [1], sets
    M, J = 18, 3
    x = [rng.uniform(size=(M, 2)), [None]]
    out = _replay(monkeypatch, sysm, x, J, 10, 17, 1e-8)
    assert out[1][0].shape == (1, M, 3 * J)


# ------------------------------------------------------------------------------------------------ modes
def test_the_mode_of_the_emulators_does_not_enter_the_draw(eng, golden):
    sysm, xin = _chain(eng, golden, 'sexp')
    np.random.seed(4)
    dense = sysm.sample_paths_vecchia(xin, sample_size=3, full_layer=True, m=12)
    for mode in (True, [[True], [False], [True]], [[False], [True], [False]]):
        sysm.set_vecchia(mode)
        with pytest.raises(NotImplementedError, match='emulator 1 of layer [12]'):
            sysm.sample_paths(xin)
        np.random.seed(4)
        out = sysm.sample_paths_vecchia(xin, sample_size=3, full_layer=True, m=12)
        for l in range(3):
            close(out[l][0], dense[l][0], rtol=0, atol=0)
    sysm.set_vecchia(False)


# ------------------------------------------------------------------------------------------------ Monte Carlo
def test_full_conditioning_sets_match_the_linked_moments_by_monte_carlo(eng):
    """GP -> GP with m = 64 >= n + M - 1 at both nodes (n = 40, M = 25): the paths are exact joint draws, so the linked-GP
    moments are their mean and variance."""
    from dgp_amd.linkgp import container, lgp
    rng = np.random.default_rng(5)
    X1 = rng.uniform(size=(40, 2))
    g1 = _gp('matern2.5', X1, np.sin(4 * X1[:, :1]) + X1[:, 1:] ** 2)
    W2 = rng.uniform(-1.5, 2.0, size=(40, 1))
    g2 = _gp('sexp', W2, np.cos(2 * W2))
    sysm = lgp([[container(g1.export(), local_input_idx=np.array([0, 1]))],
                [container(g2.export(), local_input_idx=np.array([0]))]])
    x = rng.uniform(size=(25, 2))
    mu, var = sysm.predict(x)
    np.random.seed(31)
    draws = sysm.sample_paths_vecchia(x, sample_size=4000, m=64)[0][0]   # (25, 4000)
    P = draws.shape[1]
    assert P == 4000
    m_hat, v_hat = draws.mean(1), draws.var(1, ddof=1)
    print('max |mean error| / sigma_mean: %.2f (bound 5); max |variance ratio - 1| / sigma: %.2f (bound 6)'
          % (np.max(np.abs(m_hat - mu[0][:, 0]) / np.sqrt(var[0][:, 0] / P)),
             np.max(np.abs(v_hat / var[0][:, 0] - 1) / np.sqrt(2.0 / (P - 1)))))
    assert np.all(np.abs(m_hat - mu[0][:, 0]) <= 5 * np.sqrt(var[0][:, 0] / P))
    assert np.all(np.abs(v_hat / var[0][:, 0] - 1) <= 6 * np.sqrt(2.0 / (P - 1)))


# ------------------------------------------------------------------------------------------------ likelihood on top
def test_dgp_container_with_a_poisson_top(eng):
    from dgp_amd import dgp, kernel, combine, Poisson
    from dgp_amd.linkgp import container, lgp
    rng = np.random.default_rng(6)
    n = 50
    X = rng.uniform(size=(n, 2))
    K = lambda **kw: kernel(length=np.array([1.0]), name='matern2.5', nugget=1e-4, **kw)
    Y = rng.poisson(np.exp(1 + np.sin(4 * X[:, [0]]))).astype(float)
    model = dgp(X, Y, combine([K() for _ in range(2)], [K(scale_est=True)], [Poisson()]), seed=4)
    model.train(N=3, ess_burn=3, disable=True)
    np.random.seed(0)
    sysm = lgp([[container(model.estimate(), local_input_idx=np.array([0, 1]))]], N=2)
    x = rng.uniform(size=(30, 2))
    np.random.seed(3)
    dense = sysm.sample_paths(x, sample_size=5, full_layer=True)
    np.random.seed(3)
    full = sysm.sample_paths_vecchia(x, sample_size=5, full_layer=True, m=20)
    assert len(full) == len(dense) == 1 and len(full[0]) == len(dense[0])
    for a, b in zip(full[0], dense[0]):
        assert a.shape == b.shape == (1, 30, 10) and a.dtype == b.dtype
    last = full[0][0]
    assert np.all(last >= 0) and np.all(last == np.round(last))
    np.random.seed(3)
    short = sysm.sample_paths_vecchia(x, sample_size=5, m=20)
    close(short[0], last, rtol=0, atol=0)


# ------------------------------------------------------------------------------------------------ beyond the dense cap
def test_more_rows_than_the_dense_method_takes(eng):
    from dgp_amd.linkgp import container, lgp
    from dgp_amd.paths import MAX_POINTS
    rng = np.random.default_rng(12)
    X1 = rng.uniform(size=(60, 2))
    g1 = _gp('matern2.5', X1, np.sin(4 * X1[:, :1]) + X1[:, 1:] ** 2, nugget=1e-3)
    W2 = rng.uniform(-1.5, 2.5, size=(50, 1))
    g2 = _gp('sexp', W2, np.cos(2 * W2), nugget=1e-3)
    sysm = lgp([[container(g1.export(), local_input_idx=np.array([0, 1]))],
                [container(g2.export(), local_input_idx=np.array([0]))]])
    M = 20000
    assert M > MAX_POINTS
    big = rng.uniform(size=(M, 2))
    with pytest.raises(ValueError):
        sysm.sample_paths(big, sample_size=2)
    np.random.seed(1)
    out = sysm.sample_paths_vecchia(big, sample_size=2, full_layer=True)
    assert [len(o) for o in out] == [1, 1]
    for o in out:
        assert o[0].shape == (1, M, 2) and np.all(np.isfinite(o[0]))


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_nothing_behind(eng, golden):
    import torch
    sysm, xin = _chain(eng, golden, 'sexp')
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    with pytest.raises(Exception, match='numpy 2d-array'):
        sysm.sample_paths_vecchia(xin[0][:, 0])
    with pytest.raises(Exception, match='global inputs to the all layers'):
        sysm.sample_paths_vecchia(xin[:2])
    with pytest.raises(ValueError):
        sysm.sample_paths_vecchia(xin, m=0)
    assert torch.cuda.memory_allocated() == before


def test_a_block_that_does_not_factor_names_its_place(eng):
    """The indefinite node of the dense refusal test (a repeated input row, a slightly negative nugget): the jitter policy
    of vpaths either repairs the block with a warning or gives up with LinAlgError, and both name the place."""
    from dgp_amd import kernel
    from dgp_amd.linkgp import container, lgp
    rng = np.random.default_rng(2)
    n = 40
    X = rng.uniform(size=(n, 2))
    X[17] = X[4]
    y = np.sin(4 * X[:, 0]) + X[:, 1]
    y[17] = y[4]
    nd = kernel(length=np.array([0.6, 0.9]), name='matern2.5', nugget=-1e-3, scale=1.7)
    nd.input, nd.output, nd.global_input, nd.engine = X, y[:, None], None, eng
    nd.input_dim, nd.D = np.arange(2), 2
    c = container.__new__(container)
    c.type, c.structure, c.vecch, c.local_input_idx = 'gp', nd, False, np.arange(2)
    bad = lgp.__new__(lgp)
    bad.L, bad.all_layer, bad.num_model, bad.all_layer_set = 1, [[c]], [], [[[copy.copy(c)]]]
    x = np.concatenate((X[[4]] + 1e-9, rng.uniform(size=(8, 2))))
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        try:
            out = bad.sample_paths_vecchia(x, sample_size=3, m=45)
            assert np.all(np.isfinite(out[0]))
            assert any('did not factor' in str(w.message) and 'layer 1, emulator 1, system 1' in str(w.message) for w in rec)
        except np.linalg.LinAlgError as err:
            assert 'layer 1, emulator 1, system 1' in str(err)
