"""Joint sample paths of linked systems (lgp.sample_paths).  Needs an MI355X: -m gpu.

The replays walk every path of the system in numpy with the same normals, each GP node by the joint Cholesky of
tests/test_gpu_sample_paths.py (no inverse formed, a different route from the device's L^-1)."""
import copy

import numpy as np
import pytest

from test_gpu_sample_paths import _gp, close, ref_path

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    from dgp_amd.ops import Engine
    return Engine(0)


def _node_path(nd, xin, eps):
    return ref_path(nd._X(), xin, np.asarray(nd.output, float).reshape(1, -1), nd.length, nd.nugget[0], nd.scale[0],
                    nd.name, eps, None if nd.rep is None else nd.W_diag)


def _dgp_paths(struct, m, z, l, J, s, Zit):
    """Paths (J, M, q) of one DGP emulator of system s, input m (J, M, D), external z: as lgp.sample_paths documents."""
    L = len(struct)
    internal, external = struct[0][0].input_dim, struct[0][0].connect
    prev = None
    for il, layer in enumerate(struct):
        cur = np.empty(m.shape[:2] + (len(layer),))
        for j, nd in enumerate(layer):
            if nd.type != 'gp':
                continue
            eps = next(Zit)[s]
            for p in range(J):
                if il == 0:
                    xin = m[p] if z is None else np.concatenate((m[p], z), 1)
                else:
                    parts = [prev[p][:, nd.input_dim]]
                    if nd.connect is not None and l == 0:
                        parts.append(m[p][:, nd.connect])
                    elif nd.connect is not None:
                        if il == L - 1:
                            i1 = np.where(nd.connect[:, None] == internal[None, :])[1]
                            i2 = np.array([], int) if external is None else np.where(nd.connect[:, None] == external[None, :])[1]
                        else:
                            D = m.shape[2]
                            i1, i2 = nd.connect[nd.connect <= D - 1], nd.connect[nd.connect > D - 1] - D
                        parts += [m[p][:, i1]] + ([z[:, i2]] if i2.size else [])
                    xin = np.concatenate(parts, 1)
                cur[p, :, j] = _node_path(nd, xin, eps[p])
        prev = cur
    return prev


def _walk(sysm, x, J, Z):
    """Per layer, per emulator, the (q, M, S*J) paths of the system; Z: the GP nodes' (S, J, M) normals in walk order."""
    S = len(sysm.all_layer_set)
    M = len(x[0])
    out = [[None] * len(layer) for layer in sysm.all_layer]
    feed = []
    for l, layer in enumerate(sysm.all_layer):
        Zs = {}   # per emulator, its blocks of normals (the same for every system)
        per_sys = []
        for s, one in enumerate(sysm.all_layer_set):
            Zit = iter(Z[l])
            outs = []
            for k, c in enumerate(one[l]):
                idx = c.local_input_idx
                if l == 0:
                    m = np.broadcast_to(x[0][:, idx], (J, M, len(idx)))
                else:
                    idx = idx if isinstance(idx, list) else [None] * (l - 1) + [idx]
                    m = np.concatenate([feed[i][s][:, :, j] for i, j in enumerate(idx) if j is not None], 2)
                z = None if l == 0 else x[l][k]
                if c.type == 'gp':
                    eps = next(Zit)[s]
                    o = np.stack([_node_path(c.structure, m[p] if z is None else np.concatenate((m[p], z), 1), eps[p])
                                  for p in range(J)])[:, :, None]
                else:
                    o = _dgp_paths(c.structure, m, z, l, J, s, Zit)
                outs.append(o)
            per_sys.append(outs)
        feed.append([np.concatenate(o, 2) for o in per_sys])
        for k in range(len(layer)):
            out[l][k] = np.concatenate([per_sys[s][k] for s in range(S)], 0).transpose(2, 1, 0)
    return out


def _normals(sysm, M, J, seed):
    """The GP nodes' normals in walk order, grouped by layer of the system."""
    np.random.seed(seed)
    S = len(sysm.all_layer_set)
    Z = []
    for l, layer in enumerate(sysm.all_layer):
        zl = []
        for c in layer:
            nodes = [c.structure] if c.type == 'gp' else [nd for lay in c.structure for nd in lay]
            zl += [np.random.standard_normal((S, J, M)) for nd in nodes if nd.type == 'gp']
        Z.append(zl)
    return Z


# ------------------------------------------------------------------------------------------------ one GP container
@pytest.mark.parametrize('case', ['plain', 'connect', 'replicates'])
@pytest.mark.parametrize('kind', ['sexp', 'matern2.5'])
def test_one_gp_container_equals_gp_sample_paths(eng, kind, case):
    from dgp_amd.linkgp import container, lgp
    rng = np.random.default_rng(11)
    X = rng.uniform(size=(60, 3))
    if case == 'replicates':
        X = np.concatenate((X, X[:15]))
    Y = (np.sin(3 * X[:, 0]) + X[:, 1] * X[:, 2] + 0.05 * rng.normal(size=len(X)))[:, None]
    m = _gp(kind, X, Y, connect=np.array([2]) if case == 'connect' else None)
    cols = np.array([0, 1, 2])   # (input_dim then connect: [0, 1] + [2] in the connect case)
    sysm = lgp([[container(m.export(), local_input_idx=cols)]])
    assert len(sysm.all_layer_set) == 1
    xt = rng.uniform(size=(35, 3))
    np.random.seed(21)
    ref = m.sample_paths(xt, sample_size=7)
    np.random.seed(21)
    out = sysm.sample_paths(xt, sample_size=7)
    assert len(out) == 1 and out[0].shape == (1, 35, 7)
    close(out[0][0], ref, rtol=1e-12, atol=1e-12 * np.sqrt(m.kernel.scale[0]))


# ------------------------------------------------------------------------------------------------ GP -> DGP -> GP
def _chain(eng, golden, tag):
    from test_gpu_model import build_structure
    from dgp_amd.linkgp import container, lgp
    d = golden('g10_lgp_' + tag)
    idx = [np.array([0, 1]), np.array([0]), np.array([0])]
    sets = []
    for s in range(int(d['n_imp'])):
        one = []
        for l in range(3):
            st = build_structure(d, 's%d_m%d_' % (s, l), eng)
            c = container.__new__(container)
            c.vecch, c.local_input_idx = False, idx[l]
            c.type, c.structure = ('gp', st[0][0]) if len(st) == 1 else ('dgp', st)
            one.append([c])
        sets.append(one)
    sysm = lgp.__new__(lgp)
    sysm.L, sysm.all_layer, sysm.num_model, sysm.all_layer_set = 3, sets[0], [1, 1], sets
    return sysm, [d['xt'], [None], [d['ext']]]


@pytest.mark.parametrize('tag', ['sexp', 'matern'])
def test_linked_chain_replays_the_walk(eng, golden, tag):
    sysm, xin = _chain(eng, golden, tag)
    S, M, J = len(sysm.all_layer_set), len(xin[0]), 3
    Z = _normals(sysm, M, J, 4)
    np.random.seed(4)
    out = sysm.sample_paths(xin, sample_size=J, full_layer=True)
    ref = _walk(sysm, xin, J, Z)
    assert len(out) == 3 and all(len(o) == 1 for o in out)
    for l in range(3):
        assert out[l][0].shape == ref[l][0].shape == (ref[l][0].shape[0], M, S * J)
        close(out[l][0], ref[l][0], rtol=1e-6, atol=1e-6)
    np.random.seed(4)
    short = sysm.sample_paths(xin, sample_size=J)
    assert len(short) == 1
    close(short[0], out[-1][0], rtol=0, atol=0)


# ------------------------------------------------------------------------------------------------ Monte Carlo
def test_paths_match_the_linked_moments_by_monte_carlo(eng):
    """GP -> GP: the linked-GP moments are the exact mean and variance of the propagated paths."""
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
    draws = sysm.sample_paths(x, sample_size=4000)[0][0]   # (25, 4000)
    P = draws.shape[1]
    m_hat, v_hat = draws.mean(1), draws.var(1, ddof=1)
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
    full = sysm.sample_paths(x, sample_size=5, full_layer=True)
    assert len(full) == 1 and full[0][0].shape == (1, 30, 10)
    last = full[0][0]
    assert np.all(last >= 0) and np.all(last == np.round(last))
    np.random.seed(3)
    short = sysm.sample_paths(x, sample_size=5)
    close(short[0], last, rtol=0, atol=0)


# ------------------------------------------------------------------------------------------------ wiring
def test_two_emulators_feeding_a_third_with_a_skip(eng):
    """Layer 1: A (x column 0) and B (x column 1); layer 2: C on both; layer 3: D on B (layer 1, skipping layer 2) and C,
    with an external input."""
    from dgp_amd.linkgp import container, lgp
    rng = np.random.default_rng(7)
    gA = _gp('sexp', rng.uniform(size=(30, 1)), rng.normal(size=(30, 1)))
    gB = _gp('matern2.5', rng.uniform(size=(30, 1)), rng.normal(size=(30, 1)))
    gC = _gp('matern2.5', rng.normal(size=(35, 2)), rng.normal(size=(35, 1)))
    gD = _gp('sexp', rng.normal(size=(40, 3)), rng.normal(size=(40, 1)), connect=np.array([2]))
    sysm = lgp([[container(gA.export(), local_input_idx=np.array([0])), container(gB.export(), local_input_idx=np.array([1]))],
                [container(gC.export(), local_input_idx=np.array([0, 1]))],
                [container(gD.export(), local_input_idx=[np.array([1]), np.array([0])])]])
    M, J = 20, 4
    x = [rng.uniform(size=(M, 2)), [None], [rng.uniform(size=(M, 1))]]
    Z = _normals(sysm, M, J, 9)
    np.random.seed(9)
    out = sysm.sample_paths(x, sample_size=J, full_layer=True)
    assert [len(o) for o in out] == [2, 1, 1] and all(a.shape == (1, M, J) for o in out for a in o)
    ref = _walk(sysm, x, J, Z)
    for l in range(3):
        for k in range(len(out[l])):
            close(out[l][k], ref[l][k], rtol=1e-6, atol=1e-6)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(eng, golden):
    import torch
    from dgp_amd import kernel
    from dgp_amd.linkgp import container, lgp
    from dgp_amd.paths import MAX_POINTS
    sysm, xin = _chain(eng, golden, 'sexp')
    sysm.set_vecchia(True)
    with pytest.raises(NotImplementedError, match='emulator 1 of layer 1'):
        sysm.sample_paths(xin)
    sysm.set_vecchia(False)
    rng = np.random.default_rng(2)
    before = torch.cuda.memory_allocated()
    with pytest.raises(ValueError):
        sysm.sample_paths(rng.uniform(size=(MAX_POINTS + 1, 2)))
    assert torch.cuda.memory_allocated() == before
    # the indefinite R of the emulator's refusal test (a repeated input row, a slightly negative nugget)
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
    with pytest.raises(np.linalg.LinAlgError, match=r'layer 1, emulator 1 \(gp\), system 1'):
        bad.sample_paths(rng.uniform(size=(9, 2)), sample_size=3)
