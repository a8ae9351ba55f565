"""Model-level parity on the GPU: the device imputer replays the reference's logged ESS
trajectory, the emulator reproduces the reference's predictions from dumped imputations,
and train -> estimate -> emulator -> predict recovers a step function.  -m gpu."""
import numpy as np
import pytest

from conftest import case

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


def close(a, b, rtol=1e-9, atol=1e-12):
    np.testing.assert_allclose(np.asarray(a, float), np.asarray(b, float), rtol=rtol, atol=atol)


def build_structure(d, pre, eng):
    """dgp_amd nodes from a structure dumped by oracle/gen_golden.py:dump_structure."""
    from dgp_amd import kernel
    layers = []
    for l in range(int(d[pre + 'n_layer'])):
        layer = []
        for k in range(int(d[pre + 'l%d_n' % l])):
            c = case(d, pre + 'l%d_k%d_' % (l, k))
            nd = kernel(length=c['length'].copy(), scale=c['scale'][0], nugget=c['nugget'][0], name=str(c['name']),
                        scale_est=bool(c['scale_est']), nugget_est=bool(c['nugget_est']), input_dim=c['input_dim'].copy(),
                        connect=c['connect'].copy() if bool(c['has_global']) else None, engine=eng)
            nd.input = c['input'].copy()
            nd.output = c['output'].copy()
            nd.global_input = c['global_input'].copy() if bool(c['has_global']) else None
            nd.vecch = False
            nd.D = nd.input.shape[1] + (0 if nd.global_input is None else nd.global_input.shape[1])
            layer.append(nd)
        layers.append(layer)
    return layers


@pytest.mark.parametrize('tag', ['sexp', 'matern', 'deep', 'matern200'])
@pytest.mark.parametrize('batch', [1, 3, 8])
def test_ess_trajectory_matches_reference(eng, golden, tag, batch):
    """imputer.sample with the reference's own draws: same accepted latents, and the speculative batches consume
    exactly the uniforms the sequential sampler consumed.  Every recording runs through the device-resident accept /
    shrink loop (dgpamd_ess_queue) -- the two-layer ones as one queue per I-step, 'deep' (three layers) layer by layer
    on one shared device state; 'matern200' is n = 200 (four 64-wide tiles per matrix, global input connected: panel /
    bulk tasks and the flag hand-offs of the factorisation are all on the path)."""
    from dgp_amd.imputation import imputer, DrawStream
    d = golden('g5_ess_' + tag)
    layers = build_structure(d, 'pre_', eng)
    draws = DrawStream(z=list(d['z']), u=list(d['u']))
    imp = imputer(layers, block=True, draws=draws, engine=eng, batch=batch)
    imp.sample(burnin=1 if tag == 'matern200' else 2)
    assert imp.queued_calls == 1, 'the replay must have run through the device queue'
    assert draws.exhausted(), 'all logged draws must be consumed, no more and no fewer'
    post = build_structure(d, 'post_', eng)
    for la, lb in zip(layers, post):
        for a, b in zip(la, lb):
            close(a.output, b.output, rtol=1e-8, atol=1e-10)
            close(a.input, b.input, rtol=1e-8, atol=1e-10)


@pytest.mark.parametrize('batch', [1, 5])
def test_nodewise_ess_matches_reference(eng, golden, batch):
    """block=False: imputer.one_sample per node (imputation.py:121-221) replayed with the reference's draws."""
    from dgp_amd.imputation import imputer, DrawStream
    d = golden('g5_ess_nodewise')
    layers = build_structure(d, 'pre_', eng)
    draws = DrawStream(z=list(d['z']), u=list(d['u']))
    imputer(layers, block=False, draws=draws, engine=eng, batch=batch).sample(burnin=1)
    assert draws.exhausted()
    post = build_structure(d, 'post_', eng)
    for la, lb in zip(layers, post):
        for a, b in zip(la, lb):
            close(a.output, b.output, rtol=1e-8, atol=1e-10)
            close(a.input, b.input, rtol=1e-8, atol=1e-10)


@pytest.mark.parametrize('tag', ['sexp', 'matern', 'matern150'])
def test_emulator_predict_matches_reference(eng, golden, tag):
    """emulator.predict from the reference's own imputations; 'matern150' is n = 150 (three 64-wide tiles in the
    factorisations and inverses behind compute_stats, several row tiles in the linked-GP pair kernels)."""
    from dgp_amd.emulation import emulator
    d = golden('g9_emulator_' + tag)
    S = int(d['n_imp'])
    est = build_structure(d, 's0_', eng)
    emu = emulator.__new__(emulator)
    emu.all_layer, emu.n_layer, emu.vecch, emu.engine = est, len(est), False, eng
    emu.N = emu.N_total = S
    emu.shard = False
    emu.latents = []
    for s in range(S):
        ls = build_structure(d, 's%d_' % s, eng)
        emu.latents.append([np.stack([nd.output[:, 0] for nd in layer], 1) for layer in ls[:-1]])
    emu.orders = []
    emu._stats = None
    # means go through R^-1 y: with the default nugget 1e-6 the n = 150 correlation matrices have condition ~1e7, i.e.
    # ~1e-8 of the O(1) outputs is the attainable agreement between two factorisations (the oracle itself is at 1e-8)
    am = 1e-7 if tag == 'matern150' else 1e-8
    mu_s, var_s = emu.predict(d['xt'], aggregation=False)
    for s in range(S):
        close(mu_s[s], d['mu_s'][s], rtol=1e-6, atol=am)
        # variance = O(scale) terms cancelling through R^-1 (cond ~1e6): absolute tolerance 1e-6 * prior variance
        close(var_s[s], d['var_s'][s], rtol=1e-5, atol=1e-6)
    mu, var = emu.predict(d['xt'])
    close(mu, d['mu'], rtol=1e-6, atol=am)
    close(var, d['var'], rtol=1e-5, atol=1e-6)
    ml, vl = emu.predict(d['xt'], full_layer=True)
    assert len(ml) == 2 and ml[0].shape == (len(d['xt']), 2)
    close(ml[-1], d['mu'], rtol=1e-6, atol=am)


@pytest.mark.parametrize('tag', ['sexp', 'matern'])
def test_emulator_loo_matches_reference(eng, golden, tag):
    """emulator.loo (emulation.py:109-143) from the reference's own imputations: dense emulator (all other points)
    and Vecchia emulator (m = 5)."""
    from dgp_amd.emulation import emulator
    d = golden('g14_loo_' + tag)
    S = int(d['n_imp'])
    emu = emulator.__new__(emulator)
    est = build_structure(d, 's0_', eng)
    emu.all_layer, emu.n_layer, emu.vecch, emu.engine = est, len(est), False, eng
    emu.N = emu.N_total = S
    emu.shard = False
    emu.latents = []
    for s in range(S):
        ls = build_structure(d, 's%d_' % s, eng)
        emu.latents.append([np.stack([nd.output[:, 0] for nd in layer], 1) for layer in ls[:-1]])
    emu.orders = []
    emu._stats = None
    mu, var = emu.loo(d['X'])
    close(mu, d['loo_mu'], rtol=1e-6, atol=1e-8)
    close(var, d['loo_var'], rtol=1e-5, atol=1e-7)
    assert not any(nd.loo_state for layer in emu.all_layer for nd in layer)
    emu.vecch = True
    for layer in emu.all_layer:
        for nd in layer:
            nd.vecch = True
    mu, var = emu.loo(d['X'], m=5)
    close(mu, d['loo_mu_vecch'], rtol=1e-6, atol=1e-8)
    close(var, d['loo_var_vecch'], rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize('name', ['sexp', 'matern2.5'])
def test_emulator_loo_dense_downdate_equals_refit(eng, name):
    """The dense emulator's leave-one-out walk reuses R^-1 through a rank-one downdate (dgpamd_linkgp_loo); it must
    agree with the reference's route -- every test point re-conditioned on the other n-1 points through the Vecchia
    prediction branches (emulation.py:90-108) -- on a three-layer hierarchy with a global connection, and it keeps
    working beyond the LDS limit of that route."""
    from dgp_amd import dgp, kernel, combine, emulator
    rng = np.random.default_rng(5)
    n, d = 90, 2
    X = rng.uniform(size=(n, d))
    Y = np.sin(6.0 * X[:, [0]]) * np.cos(4.0 * X[:, [1]]) + 0.5 * X[:, [1]]
    layers = combine([kernel(length=np.array([1.0]), name=name) for _ in range(d)],
                     [kernel(length=np.array([1.0]), name=name, connect=np.arange(d)) for _ in range(d)],
                     [kernel(length=np.array([1.0]), name=name, scale_est=True)])
    model = dgp(X, Y, layers, seed=2)
    model.train(N=6, ess_burn=3, disable=True)
    emu = emulator(model.estimate(), N=3, seed=11)   # (seeded: the imputations, and with them how hard the comparison is, were the
    mu, var = emu.loo(X)                             #  numpy global generator's state at this point of the test session)
    gps = [nd for layer in emu.all_layer for nd in layer if nd.type == 'gp']
    for nd in gps:
        nd.loo_state, nd.vecch = True, True
    try:
        mu_ref, var_ref = emu._aggregate(emu._layer_moments(X, 'vecchia', n))
    finally:
        for nd in gps:
            nd.loo_state, nd.vecch = False, False
    # two algebraic routes through matrices of condition ~1e8 (sexp): each carries ~1e-8 of rounding
    close(mu, mu_ref, rtol=1e-5, atol=1e-6)
    # variances are O(scale) terms cancelling through R^-1: absolute tolerance 3e-6 x prior variance (over ten sets of imputations
    # the largest difference ranged from 4e-8 to 1.06e-6, tools/gpu_loo_probe.py)
    close(var, var_ref, rtol=1e-5, atol=3e-6)
    assert np.sqrt(np.mean((mu - Y) ** 2)) < 0.2 and np.all(var > 0)
    s = emu.loo(X, method='sampling', sample_size=5)
    assert len(s) == 1 and s[0].shape == (n, 3 * 5)
    with pytest.raises(Exception, match='training input positions'):
        emu.loo(X + 1e-3)
    # a design far beyond what the re-conditioning route holds in LDS
    n2 = 600
    X2 = rng.uniform(size=(n2, d))
    Y2 = np.sin(6.0 * X2[:, [0]]) * np.cos(4.0 * X2[:, [1]]) + 0.5 * X2[:, [1]]
    model = dgp(X2, Y2, combine([kernel(length=np.array([1.0]), name=name) for _ in range(d)],
                                [kernel(length=np.array([1.0]), name=name, scale_est=True, connect=np.arange(d))]), seed=2)
    model.train(N=5, ess_burn=3, disable=True)
    emu = emulator(model.estimate(), N=2)
    mu, var = emu.loo(X2)
    pm, pv = emu.predict(X2)
    assert np.all(np.isfinite(mu)) and np.all(var > 0)
    assert np.sqrt(np.mean((mu - Y2) ** 2)) < 0.1
    assert np.mean(var) > np.mean(pv)          # leaving the point out can only lose information on average


def test_estimate_is_path_mean(eng, golden):
    """dgp.estimate (dgp.py:1529-1540)."""
    from dgp_amd.dgp import dgp
    d = golden('g9_emulator_sexp')
    layers = build_structure(d, 'est_', eng)
    for l, layer in enumerate(layers):
        for k, nd in enumerate(layer):
            nd.para_path = d['path_l%d_k%d' % (l, k)].copy()
    obj = dgp.__new__(dgp)
    obj.all_layer, obj.N = layers, 6
    est = obj.estimate()
    ref = build_structure(d, 'est_', eng)
    for la, lb in zip(est, ref):
        for a, b in zip(la, lb):
            close(a.scale, b.scale)
            close(a.length, b.length)
            close(a.nugget, b.nugget)


def test_step_function_end_to_end(eng):
    """BASELINE config 1 at its stated length: step function, n=30, 2 layers x 1 SExp node, 200 SI iterations
    (demo/step_fct.ipynb scaled as BASELINE.json states).  Statistical: the emulator must recover the two plateaus."""
    from dgp_amd import dgp, kernel, combine, emulator
    np.random.seed(3)
    n = 30
    X = np.linspace(0, 1, n)[:, None]
    Y = np.where(X > 0.5, 1.0, -1.0)
    layers = combine([kernel(length=np.array([1.0]), name='sexp')],
                     [kernel(length=np.array([1.0]), name='sexp', scale_est=True)])
    model = dgp(X, Y, layers, seed=7)
    model.train(N=200, ess_burn=10, disable=True)
    assert model.N == 200 and model.all_layer[0][0].para_path.shape == (201, 3)
    emu = emulator(model.estimate(), N=6, seed=11)
    xt = np.array([[0.1], [0.3], [0.7], [0.9]])
    mu, var = emu.predict(xt)
    assert mu.shape == (4, 1) and var.shape == (4, 1)
    assert np.all(mu[:2] < -0.7) and np.all(mu[2:] > 0.7), mu
    assert np.all(var > -1e-6) and np.all(var < 0.5)
    # the sampler's speculative batches: more than one proposal per update on average
    st = model.imp.stats
    assert st['proposals'] >= st['updates'] > 0


def test_matern_2layer_train_predict_small(eng):
    """Shape of BASELINE config 2 at a small n: d inputs -> d Matern nodes -> 1 Matern node with global connection."""
    from dgp_amd import dgp, kernel, combine, emulator
    rng = np.random.default_rng(2026)
    n, d = 120, 3
    X = rng.uniform(size=(n, d))
    f = np.sin(1.0 / ((0.7 * X[:, 0] + 0.3) * (0.7 * X[:, 1] + 0.3))) + 0.5 * X[:, 2] ** 2
    Y = ((f - f.mean()) / f.std())[:, None]
    layers = combine([kernel(length=np.array([1.0]), name='matern2.5') for _ in range(d)],
                     [kernel(length=np.array([1.0]), name='matern2.5', scale_est=True, connect=np.arange(d))])
    model = dgp(X, Y, layers, seed=1)
    model.train(N=8, ess_burn=5, disable=True)
    emu = emulator(model.estimate(), N=3, seed=2)
    mu, var = emu.predict(X[:40])
    assert np.sqrt(np.mean((mu - Y[:40]) ** 2)) < 0.3          # interpolates its own training data
    assert np.all(np.isfinite(var))
    # method='sampling' (emulation.py:780-822): D arrays of M x (N*sample_size) draws whose moments are the
    # mixture moments that method='mean_var' aggregates (emulation.py:846-847)
    smp = emu.predict(X[:40], method='sampling', sample_size=400)
    assert isinstance(smp, list) and len(smp) == 1 and smp[0].shape == (40, 3 * 400)
    sd = np.sqrt(np.maximum(var[:, 0], 1e-12))
    assert np.all(np.abs(smp[0].mean(1) - mu[:, 0]) < 6 * sd / np.sqrt(1200) + 1e-6)
    assert np.all(np.abs(smp[0].var(1) - var[:, 0]) < 0.35 * var[:, 0] + 1e-8)
    # persistence: arrays-only structure file and pickled emulator reproduce the predictions
    import os, tempfile
    from dgp_amd import save_structure, load_structure, write, read
    with tempfile.TemporaryDirectory() as tmp:
        save_structure(model.estimate(), os.path.join(tmp, 'est'))
        est2 = load_structure(os.path.join(tmp, 'est'))
        assert np.array_equal(est2[1][0].length, model.estimate()[1][0].length) and est2[1][0].scale_est
        mu2, var2 = emulator(est2, N=3, seed=2).predict(X[:40])
        assert np.allclose(mu2, mu, rtol=1e-9, atol=1e-12) and np.allclose(var2, var, rtol=1e-7, atol=1e-12)
        write(emu, os.path.join(tmp, 'emu'))
        mu3, var3 = read(os.path.join(tmp, 'emu')).predict(X[:40])
        assert np.allclose(mu3, mu, rtol=1e-9, atol=1e-12) and np.allclose(var3, var, rtol=1e-7, atol=1e-12)
    idx, best = emu.metric(X[:40], method='ALM')
    assert idx.shape == (1,) and best[0] == var[:, 0].max() and idx[0] == int(np.argmax(var[:, 0]))
    # MICE (emulation.py:377-394) against the oracle's mice_var on this emulator's own per-imputation moments
    from oracle import dgp_oracle as O
    xc = X[:40]
    score = emu.metric(xc, method='MICE', nugget_s=1.0, score_only=True)
    pl = [(a.cpu().numpy(), b.cpu().numpy()) for a, b in emu._layer_moments(xc)]
    nd = emu.all_layer[-1][0]
    ref = np.zeros((40, 1))
    for i in range(emu.N):
        ref += np.log(pl[-1][1][i] / O.mice_var(pl[-2][0][i], xc, nd.input_dim, nd.connect, nd.name, nd.length, nd.scale,
                                                 nd.nugget[0], 1.0))
    assert np.allclose(score, ref / emu.N, rtol=1e-8, atol=1e-10)
    # VIGF (emulation.py:396-420) from the same per-imputation moments
    vig = emu.metric(xc, method='VIGF', obj=model, score_only=True)
    nearest = np.argmin(((xc[:, None, :] - model.X[None]) ** 2).sum(-1), 1)
    b = (pl[-1][0] - model.all_layer[-1][0].output[nearest][None, :, :]) ** 2
    ref_v = np.mean(b ** 2 + 6 * b * pl[-1][1] + 3 * pl[-1][1] ** 2, 0) - np.mean(b + pl[-1][1], 0) ** 2
    assert vig.shape == (40, 1) and np.allclose(vig, ref_v, rtol=1e-10, atol=1e-14)
    idx2, best2 = emu.metric(xc, method='MICE')
    assert idx2[0] == int(np.argmax(score[:, 0])) and best2[0] == score[:, 0].max()
    full = emu.predict(X[:10], method='sampling', sample_size=5, full_layer=True)
    assert len(full) == 2 and len(full[0]) == d and full[0][0].shape == (10, 15) and full[1][0].shape == (10, 15)
    mu_l, var_l = emu.predict(X[:10], full_layer=True)
    assert len(mu_l) == 2 and mu_l[0].shape == (10, d) and np.allclose(mu_l[1], mu[:10], rtol=1e-9, atol=1e-12)


def test_lost_handoff_retry_leaves_the_paths_as_one_iteration_does(eng):
    """dgp.train repeats an iteration whose one-launch factorisation lost a hand-off (HandoffError) through the per-block-step
    kernel.  What the interrupted attempt had already committed must not stay: nodes fitted before the failure have appended a
    row to para_path (estimate()'s burn-in index and reinit_all_layer(row=...) count rows), and the M-step's hand-over to the
    imputer (_adopt / _adopt_ll) belongs to the aborted state.  Injected: the first M-step of a run completes, then raises."""
    import warnings
    from dgp_amd import dgp, kernel, combine
    from dgp_amd.ops import HandoffError
    rng = np.random.default_rng(5)
    n, d = 90, 2
    X = rng.uniform(size=(n, d))
    Y = (np.sin(5 * X[:, :1]) + X[:, 1:] ** 2)
    Y = (Y - Y.mean()) / Y.std()
    layers = combine([kernel(length=np.array([1.0]), name='matern2.5') for _ in range(d)],
                     [kernel(length=np.array([1.0]), name='matern2.5', scale_est=True, connect=np.arange(d))])
    model = dgp(X, Y, layers, seed=3)
    nodes = [nd for layer in model.all_layer for nd in layer if nd.type == 'gp']
    rows0 = [len(nd.para_path) for nd in nodes]
    orig, calls = model._m_step, {'n': 0}

    def failing(*a, **k):
        calls['n'] += 1
        r = orig(*a, **k)
        if calls['n'] == 1:
            raise HandoffError('injected: a bounded in-kernel spin ran out')
        return r
    model._m_step = failing
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter('always')
            model.train(N=3, ess_burn=3, disable=True)
        assert any('one launch per block step' in str(x.message) for x in w)
        assert calls['n'] == 4                                   # iteration 1 twice, then 2 and 3
        assert [len(nd.para_path) for nd in nodes] == [r + 3 for r in rows0]
        assert '_adopt_ll' not in model.imp.__dict__ or model.imp.__dict__['_adopt_ll'] is not None   # (whatever is there is the LAST M-step's)
        assert model.engine.potrf_mode() == 0 if hasattr(model.engine, 'potrf_mode') else True
        est = model.estimate()
        assert all(np.all(np.isfinite(nd.length)) for layer in est for nd in layer if nd.type == 'gp')
    finally:
        model._m_step = orig
        model.engine.set_potrf_mode(1)


def test_vecchia_train_predict_end_to_end(eng):
    """Vecchia mode through the public API: ordering + ordered NN on device, fmvn_sp prior draws,
    vecchia_llik ESS targets, vecchia_nllik M-step, NN refresh at iterations 2,4,.., Vecchia prediction."""
    from dgp_amd import dgp, kernel, combine, emulator
    np.random.seed(5)
    rng = np.random.default_rng(5)
    n, d = 400, 2
    X = rng.uniform(size=(n, d))
    f = np.sin(5 * X[:, 0]) * np.cos(3 * X[:, 1])
    Y = ((f - f.mean()) / f.std())[:, None]
    layers = combine([kernel(length=np.array([1.0]), name='sexp') for _ in range(d)],
                     [kernel(length=np.array([1.0]), name='sexp', scale_est=True, connect=np.arange(d))])
    model = dgp(X, Y, layers, vecchia=True, m=15, seed=3)
    nd = model.all_layer[0][0]
    assert nd.vecch and nd.NNarray.shape == (n, 16) and nd.NNarray.dtype == np.int64
    assert np.array_equal(np.sort(nd.ord), np.arange(n)) and np.array_equal(nd.ord[nd.rev_ord], np.arange(n))
    model.train(N=4, ess_burn=3, disable=True)
    assert model.all_layer[1][0].para_path.shape[0] == 5
    emu = emulator(model.estimate(), N=2, seed=4)
    mu, var = emu.predict(X[:50], m=30)
    assert mu.shape == (50, 1) and np.all(np.isfinite(mu)) and np.all(var > -1e-8)
    assert np.sqrt(np.mean((mu - Y[:50]) ** 2)) < 0.35
    smp = emu.predict(X[:20], m=30, method='sampling', sample_size=7)
    assert len(smp) == 1 and smp[0].shape == (20, 14) and np.all(np.isfinite(smp[0]))
    mu_l, var_l = emu.predict(X[:20], m=30, full_layer=True)
    assert len(mu_l) == 2 and mu_l[0].shape == (20, d) and np.allclose(mu_l[1], mu[:20], rtol=1e-9, atol=1e-12)


def test_vecchia_llik_matches_dense_when_m_is_full(eng):
    """With m = n-1 the Vecchia likelihood is the exact Gaussian log-likelihood, up to the n log(scale) term that
    the reference's vecchia_llik leaves out (vecchia.py:179 vs kernel_class.py:482-488; it cancels in the ESS test)."""
    from dgp_amd import kernel
    rng = np.random.default_rng(9)
    n = 60
    nd = kernel(length=np.array([0.7, 1.1]), scale=1.3, nugget=1e-3, name='matern2.5', engine=eng)
    nd.input = rng.uniform(size=(n, 2))
    nd.output = rng.normal(size=(n, 1))
    dense = float(np.ravel(nd.log_likelihood_func())[0])
    nd.vecch, nd.m = True, n - 1
    nd.ord_nn()
    close(np.ravel(nd.log_likelihood_func_vecch())[0], dense + 0.5 * n * np.log(1.3), rtol=1e-9)


@pytest.mark.parametrize('tag', ['sexp', 'matern'])
def test_linked_chain_matches_reference(eng, golden, tag):
    """BASELINE config 5 shape at small n: GP -> DGP -> GP (+ external input), lgp.predict (linkgp.py:285-501)
    from the reference's dumped imputations; the DGP's second layer sees its uncertain global input through
    linkgp_prediction_full (kernel_class.py:672-733)."""
    from dgp_amd.linkgp import container, lgp
    d = golden('g10_lgp_' + tag)
    S = int(d['n_imp'])
    idx = [np.array([0, 1]), np.array([0]), np.array([0])]
    sets = []
    for s in range(S):
        one = []
        for l in range(3):
            st = build_structure(d, 's%d_m%d_' % (s, l), eng)
            c = container.__new__(container)
            c.vecch, c.local_input_idx = False, idx[l]
            if len(st) == 1:
                c.type, c.structure = 'gp', st[0][0]
            else:
                c.type, c.structure = 'dgp', st
            one.append([c])
        sets.append(one)
    sysm = lgp.__new__(lgp)
    sysm.L, sysm.all_layer, sysm.num_model, sysm.all_layer_set = 3, sets[0], [1, 1], sets
    xin = [d['xt'], [None], [d['ext']]]
    mu, var = sysm.predict(xin)
    close(mu[0], d['mu'], rtol=1e-6, atol=1e-8)
    close(var[0], d['var'], rtol=1e-5, atol=1e-6)
    mul, varl = sysm.predict(xin, full_layer=True)
    for l in range(3):
        close(mul[l][0], d['mu_l%d' % l], rtol=1e-6, atol=1e-8)
        close(varl[l][0], d['var_l%d' % l], rtol=1e-5, atol=1e-6)
    # method='sampling' (linkgp.py:348-500): draws whose moments are the mixture's
    np.random.seed(3)
    smp = sysm.predict(xin, method='sampling', sample_size=400)
    assert len(smp) == 1 and smp[0].shape == (1, len(d['xt']), S * 400)
    sd = np.sqrt(d['var'][:, 0])
    assert np.all(np.abs(smp[0][0].mean(1) - d['mu'][:, 0]) < 6 * sd / np.sqrt(S * 400) + 1e-6)
    full = sysm.predict(xin, method='sampling', sample_size=3, full_layer=True)
    assert len(full) == 3 and full[0][0].shape[2] == S * 3
    # lgp.set_vecchia (linkgp.py:180-212): with every training point in the conditioning set the Vecchia predictions are
    # the dense ones up to rounding; switching back restores them
    sysm.set_vecchia(True)
    assert all(c.vecch for one in sysm.all_layer_set for layer in one for c in layer)
    mu_v, var_v = sysm.predict(xin, m=len(d['X1']))
    close(mu_v[0], d['mu'], rtol=1e-5, atol=1e-6)
    sysm.set_vecchia([[False], [False], [False]])
    mu_d, var_d = sysm.predict(xin)
    close(mu_d[0], d['mu'], rtol=1e-6, atol=1e-8)


def test_gp_class_predict_matches_reference(eng, golden):
    """gp.predict (gp.py:412-453) at the reference's trained hyper-parameters; and gp.train() improves the objective."""
    from dgp_amd import gp, kernel
    d = golden('g10_lgp_matern')
    est = d['gp1_path'][-1]
    k = kernel(length=est[1:-1].copy(), scale=est[0], nugget=est[-1], name='matern2.5', scale_est=True)
    model = gp(d['X1'], d['Y1'], k)
    mu, var = model.predict(d['xt'])
    close(mu, d['gp1_mu'], rtol=1e-7, atol=1e-9)
    close(var, d['gp1_var'], rtol=1e-5, atol=1e-7)
    k2 = kernel(length=np.array([0.8, 1.2]), name='matern2.5', scale_est=True, nugget=1e-4)
    m2 = gp(d['X1'], d['Y1'], k2)
    before = float(k2.llik(k2.log_t())[0][0])
    m2.train()
    after = float(k2.llik(k2.log_t())[0][0])
    assert after <= before + 1e-9 and k2.para_path.shape == (2, 4)
    assert len(m2.export()) == 1
    smp = m2.predict(d['xt'], method='sampling', sample_size=7)
    assert smp.shape == (len(d['xt']), 7)


def test_gp_loo_vecchia_matches_reference(eng, golden):
    """gp.loo under Vecchia (gp.py:345-353, vecchia.py:656-674) without and with replicated inputs."""
    from dgp_amd import gp, kernel
    g = golden('g14_loo_gp')
    for c in range(2):
        k = kernel(length=g['c%d_length' % c].copy(), scale=g['c%d_scale' % c][0], nugget=g['c%d_nugget' % c][0],
                   name=str(g['c%d_name' % c]), scale_est=True, nugget_est=True)
        model = gp(g['c%d_X' % c], g['c%d_Y' % c], k, vecchia=True, m=8)
        mu, s2 = model.loo(m=6)
        close(mu, g['c%d_mu' % c], rtol=1e-8, atol=1e-10)
        close(s2, g['c%d_s2' % c], rtol=1e-7, atol=1e-10)
        assert model.loo(method='sampling', sample_size=4, m=6).shape == (len(g['c%d_X' % c]), 4)


def test_hetero_exact_posterior_draw(eng, golden):
    """Engine.post_het (the device form of Hetero.post_het1 / post_het2) against the reference's draws (g13_hetero)."""
    from oracle import dgp_oracle as O
    from dgp_amd import Hetero
    g = golden('g13_hetero')
    v = g['a_v']
    f1 = eng.post_het(eng.tensor(v), 1.0, eng.tensor(g['a_Gamma']), eng.tensor(g['a_y'].flatten()), eng.tensor(g['a_z1']))
    close(npy(f1), g['a_f1'], rtol=1e-8, atol=1e-10)
    h = Hetero()
    h.rep = g['a_mask']
    h.input = np.stack((np.zeros(len(g['a_mask'])), np.log(g['a_Gamma2'])), 1)
    h.output = g['a_y2']
    f2 = h.posterior(np.array([0]), v, sd=g['a_z2'], engine=eng)
    close(f2, g['a_f2'], rtol=1e-8, atol=1e-10)
    # the same through scale * K with the kernel matrix assembled on the device
    K = eng.kmatrix('matern2.5', eng.tensor(g['a_X']), None, None, g['a_length'], g['a_nugget'][0])
    f1b = eng.post_het(K, g['a_scale'][0], eng.tensor(g['a_Gamma']), eng.tensor(g['a_y'].flatten()), eng.tensor(g['a_z1']))
    close(npy(f1b), g['a_f1'], rtol=1e-8, atol=1e-10)
    close(h.llik(), O.hetero_llik(h.input, h.output), rtol=1e-13)


@pytest.mark.parametrize('tag', ['norep', 'rep'])
def test_hetero_sampler_matches_reference(eng, golden, tag):
    """imputer.sample(burnin=2) of a (2 GP nodes -> Hetero) hierarchy with the reference's own draws: the mean latent
    from its exact conditional posterior, the log-variance latent by ESS against the likelihood (imputation.py:121-221)."""
    from dgp_amd import Hetero
    from dgp_amd.imputation import imputer, DrawStream
    g = golden('g13_hetero')
    pre = 'c_%s_' % tag
    layer1 = build_structure(g, pre + 'pre_', eng)[0]
    lik = Hetero(input_dim=g[pre + 'pre_lik_input_dim'].copy())
    lik.input, lik.output = g[pre + 'pre_lik_input'].copy(), g[pre + 'pre_lik_output'].copy()
    lik.rep = g[pre + 'pre_lik_rep'].copy() if bool(g[pre + 'pre_lik_has_rep']) else None
    z, zh = g[pre + 'z'], g[pre + 'zh']
    zs = []
    for i in range(len(zh)):     # per sweep: posterior normals of node 0, then the prior draw of node 1
        zs.append(zh[i])
        zs.append(z[i])
    imp = imputer([layer1, [lik]], block=True, draws=DrawStream(z=zs, u=list(g[pre + 'u'])), engine=eng, batch=3)
    imp.sample(burnin=2)
    assert imp.draws.exhausted()
    post = build_structure(g, pre + 'post_', eng)[0]
    for a, b in zip(layer1, post):
        close(a.output, b.output, rtol=1e-7, atol=1e-9)
    close(lik.input, g[pre + 'post_lik_input'], rtol=1e-7, atol=1e-9)


@pytest.mark.parametrize('rep', [False, True])
def test_hetero_dgp_end_to_end(eng, rep):
    """A heteroskedastic DGP through the public API (dgp.py:163-246 warm start, node-wise sampler with the exact
    posterior step, M-step over the two GP nodes): the learnt noise level must follow the truth."""
    from dgp_amd import dgp, kernel, combine, Hetero
    rng = np.random.default_rng(4)
    np.random.seed(4)
    x = np.sort(rng.uniform(size=45 if rep else 90))
    if rep:
        x = np.repeat(x, np.tile([1, 2, 3], 15))     # (sites observed once exercise the singleton branch of the warm start)
    X = x[:, None]
    sd = 0.05 + 0.5 * x ** 2
    Y = (np.sin(6 * x) + sd * rng.normal(size=len(x)))[:, None]
    layers = combine([kernel(length=np.array([0.5]), name='sexp', scale_est=True),
                      kernel(length=np.array([0.5]), name='sexp', scale_est=True)], [Hetero()])   # as in the reference's demo
    model = dgp(X, Y, layers, seed=2)
    lik = model.all_layer[1][0]
    assert (lik.rep is not None) == rep and lik.input.shape == (len(x), 2)
    model.train(N=40, ess_burn=5, disable=True)
    assert model.all_layer[0][0].para_path.shape[0] == 41 and np.all(np.isfinite(model.all_layer[0][1].para_path))
    mean_lat, logvar_lat = model.all_layer[0][0].output[:, 0], model.all_layer[0][1].output[:, 0]
    xs = model.X[:, 0]
    assert np.sqrt(np.mean((mean_lat - np.sin(6 * xs)) ** 2)) < 0.25
    lo, hi = xs < 0.3, xs > 0.75
    assert np.mean(logvar_lat[hi]) > np.mean(logvar_lat[lo]) + 1.0      # noise grows with x (log-variance gap ~4)
    if not rep:
        # emulator with the likelihood on top: predictive moments of y (Hetero.prediction), sampling, nllik
        from dgp_amd import emulator
        from dgp_amd.likelihood_class import ghdiag
        from oracle import dgp_oracle as O
        emu = emulator(model.estimate(), N=4, seed=5)
        xt = np.linspace(0.05, 0.95, 19)[:, None]
        mu, var = emu.predict(xt)
        assert mu.shape == (19, 1) and np.sqrt(np.mean((mu[:, 0] - np.sin(6 * xt[:, 0])) ** 2)) < 0.3
        assert var[xt[:, 0] > 0.75].mean() > 4 * var[xt[:, 0] < 0.3].mean()       # sd 0.33-0.5 against 0.05-0.1
        mu_l, var_l = emu.predict(xt, full_layer=True)
        assert len(mu_l) == 2 and mu_l[0].shape == (19, 2) and np.allclose(mu_l[1], mu)
        smp = emu.predict(xt, method='sampling', sample_size=300)
        assert len(smp) == 1 and smp[0].shape == (19, 1200)
        assert np.all(np.abs(smp[0].mean(1) - mu[:, 0]) < 6 * np.sqrt(var[:, 0] / 1200) + 1e-3)
        yt = (np.sin(6 * xt[:, 0]) + (0.05 + 0.5 * xt[:, 0] ** 2) * rng.normal(size=19))[:, None]
        avg, per = emu.nllik(xt, yt)
        assert per.shape == (19,) and np.isfinite(avg) and avg < 1.0
        m_, v_ = rng.normal(size=(6, 2)), rng.uniform(0.1, 1.0, size=(6, 2))
        y_ = rng.normal(size=(6, 1))
        assert np.allclose(ghdiag(Hetero.pllik, m_, v_, y_), O.ghdiag(O.hetero_pllik, m_, v_, y_), rtol=1e-13)
        # sequential-design criteria under a likelihood act on the last GP layer (emulation.py:347-420,498-524)
        pl = [(a.cpu().numpy(), b.cpu().numpy()) for a, b in emu._layer_moments(xt)]
        alm = emu.metric(xt, method='ALM', score_only=True)
        mbar = pl[0][0].mean(0)
        assert alm.shape == (19, 2) and np.allclose(alm, (pl[0][0] ** 2 + pl[0][1]).mean(0) - mbar ** 2, rtol=1e-9)
        mice = emu.metric(xt, method='MICE', score_only=True)
        ref = np.stack([pl[0][1][0][:, k] / np.ravel(O.mice_var(xt, xt, nd.input_dim, nd.connect, nd.name, nd.length, nd.scale, nd.nugget[0], 1.0))
                        for k, nd in enumerate(emu.all_layer[0])], 1)
        assert np.allclose(mice, ref, rtol=1e-8)
        vig = emu.metric(xt, method='VIGF', obj=model, score_only=True)
        near = np.argmin(((xt[:, None, :] - model.X[None]) ** 2).sum(-1), 1)
        b = (pl[0][0] - np.stack([emu.latents[s_][0][near] for s_ in range(emu.N)])) ** 2
        assert np.allclose(vig, np.mean(b ** 2 + 6 * b * pl[0][1] + 3 * pl[0][1] ** 2, 0) - np.mean(b + pl[0][1], 0) ** 2, rtol=1e-10)


def test_update_xy_warm_starts(eng):
    """dgp.update_xy (dgp.py:824-1095), the sequential-design entry point: superset -> hidden latents kept at the
    old sites and set to the nodes' GP conditional means at the new ones (checked against the oracle's gp_predict),
    subset -> latents subsetted, unrelated design -> fresh warm start, reset=True -> hyper-parameters back to the
    initial ones; training and prediction keep working afterwards."""
    from dgp_amd import dgp, kernel, combine, emulator
    from oracle import dgp_oracle as O
    rng = np.random.default_rng(77)
    d = 2
    fun = lambda X: np.sin(5.0 * X[:, [0]]) * np.cos(3.0 * X[:, [1]])
    X = rng.uniform(size=(48, d))
    Y = fun(X)
    layers = combine([kernel(length=np.array([1.0]), name='matern2.5') for _ in range(d)],
                     [kernel(length=np.array([1.0]), name='matern2.5', scale_est=True, connect=np.arange(d))])
    model = dgp(X[:40], Y[:40], layers, seed=3)
    model.train(N=4, ess_burn=3, disable=True)
    # --- superset: the warm start itself (before any sampling), node by node
    old_out = [nd.output.copy() for nd in model.all_layer[0]]
    old_in = [nd.input.copy() for nd in model.all_layer[0]]
    hyp = [(nd.length.copy(), nd.nugget[0], nd.scale[0]) for nd in model.all_layer[0]]
    model.Y, model.X, model.indices = Y, X, None
    model.n_data = len(X)
    sub = np.arange(40)
    model._update_all_layer_larger(sub)
    for k, nd in enumerate(model.all_layer[0]):
        assert nd.input.shape == (48, d) and nd.output.shape == (48, 1)
        assert np.array_equal(nd.output[:40], old_out[k])
        st = O.compute_stats(old_in[k], old_out[k].ravel(), hyp[k][0], hyp[k][1], 'matern2.5', d)
        mref, _ = O.gp_predict(X[40:, nd.input_dim], old_in[k], st['Rinv'], st['Rinv_y'], hyp[k][2], hyp[k][0], hyp[k][1], 'matern2.5')
        close(nd.output[40:, 0], mref, rtol=1e-7, atol=1e-9)
    top = model.all_layer[1][0]
    assert top.input.shape == (48, d) and top.global_input.shape == (48, d) and np.array_equal(top.output, Y)
    assert np.array_equal(top.input, np.concatenate([nd.output for nd in model.all_layer[0]], 1))
    # --- the public call: superset, subset, unrelated, reset
    model = dgp(X[:40], Y[:40], combine([kernel(length=np.array([1.0]), name='matern2.5') for _ in range(d)],
                                        [kernel(length=np.array([1.0]), name='matern2.5', scale_est=True, connect=np.arange(d))]), seed=3)
    model.train(N=4, ess_burn=3, disable=True)
    len_before = model.all_layer[1][0].length.copy()
    model.update_xy(X, Y)
    assert model.n_data == 48 and model.all_layer[0][0].output.shape == (48, 1) and model.N == 4
    assert np.array_equal(model.all_layer[1][0].length, len_before)          # hyper-parameters carried over
    model.train(N=2, ess_burn=3, disable=True)
    assert model.all_layer[1][0].para_path.shape[0] == 1 + 6
    keep = np.array([3, 0, 17, 45, 21, 9, 30, 41, 12, 5, 28, 33])
    model.update_xy(X[keep], Y[keep])
    assert model.n_data == 12 and model.all_layer[1][0].input.shape == (12, d)
    assert np.array_equal(model.X, X[keep]) and model.all_layer[0][1].output.shape == (12, 1)
    assert np.array_equal(model.all_layer[1][0].global_input, X[keep]) and np.array_equal(model.all_layer[1][0].output, Y[keep])
    # the subsetting itself (before any sampling)
    m2 = dgp(X, Y, combine([kernel(length=np.array([1.0]), name='matern2.5') for _ in range(d)],
                           [kernel(length=np.array([1.0]), name='matern2.5', scale_est=True, connect=np.arange(d))]), seed=4)
    lat2 = [nd.output.copy() for nd in m2.all_layer[0]]
    m2.X, m2.Y, m2.n_data = X[keep], Y[keep], 12
    m2._update_all_layer_smaller(keep)
    for k, nd in enumerate(m2.all_layer[0]):
        assert np.array_equal(nd.output, lat2[k][keep]) and np.array_equal(nd.input, X[keep])
    assert np.array_equal(m2.all_layer[1][0].input, np.concatenate([a[keep] for a in lat2], 1))
    Xn = rng.uniform(size=(30, d))
    model.update_xy(Xn, fun(Xn))
    assert model.n_data == 30 and np.all(np.isfinite(model.all_layer[0][0].output))
    model.train(N=2, ess_burn=3, disable=True)
    model.update_xy(Xn, fun(Xn), reset=True)
    assert np.array_equal(model.all_layer[1][0].length, np.array([1.0])) and model.all_layer[1][0].para_path.shape[0] == 1 + model.N
    model.train(N=3, ess_burn=3, disable=True)
    mu, var = emulator(model.estimate(), N=2, seed=1).predict(Xn[:10])
    assert mu.shape == (10, 1) and np.all(np.isfinite(mu)) and np.all(var > 0)
    # update_all_layer (dgp.py:760-822): continue from an estimated structure
    est = model.estimate()
    model.update_all_layer(est)
    assert model.N == 0 and model.all_layer is est and est[1][0].para_path.shape == (1, 3 + 0)
    model.train(N=2, ess_burn=2, disable=True)
    assert est[1][0].para_path.shape[0] == 3


def test_hetero_vecchia_posterior_matches_reference(eng, golden):
    """Engine.vecchia_post_het (dgpamd_vecchia_het_rows + two sparse solves) against the reference's draws
    (g15_hetero_vecchia: kernel_class.py:268-275, vecchia.py:426-446,599-610, likelihood_class.py:153-182),
    and kernel.ord_nn(pointer=True) reproduces the reference's imp_NNarray."""
    import torch
    from dgp_amd import kernel
    g = golden('g15_hetero_vecchia')
    for c in range(2):
        d = case(g, 'c%d_' % c)
        X, ord_, m = d['X'], d['ord'], int(d['m'])
        n = len(X)
        length, scale, name = d['length'], d['scale'][0], str(d['name'])
        k = kernel(length=length.copy(), scale=scale, nugget=1e-6, name=name, engine=eng)
        k.input, k.global_input, k.m = X, None, m
        k.ord_nn(ord=ord_, NNarray=np.zeros((n, m + 1), np.int64), pointer=True)
        assert np.array_equal(k.imp_NNarray, d['impNN'])
        lik_in, y = d['lik_input'], d['lik_output'].ravel()
        if bool(d['has_rep']):
            invG = 1.0 / np.exp(lik_in[:, 1])
            gam = 1.0 / np.bincount(d['rep'], weights=invG, minlength=n)
            yeff = np.bincount(d['rep'], weights=invG * y, minlength=n) * gam
        else:
            gam, yeff = np.exp(lik_in[:, 1]), y
        f = eng.vecchia_post_het(name, eng.tensor(X[ord_]), eng.tensor(k.imp_NNarray, dtype=torch.int64), scale, length,
                                 eng.tensor(gam[ord_]), eng.tensor(yeff[ord_]), eng.tensor(d['z']))
        close(npy(f)[np.argsort(ord_)], d['f'], rtol=1e-8, atol=1e-10)


@pytest.mark.parametrize('rep', [False, True])
def test_hetero_dgp_vecchia_end_to_end(eng, rep):
    """The heteroskedastic DGP of test_hetero_dgp_end_to_end in Vecchia mode: warm start through gp.loo under
    Vecchia, node-wise sampler with the sparse exact-posterior step, Vecchia M-step."""
    from dgp_amd import dgp, kernel, combine, Hetero, emulator
    rng = np.random.default_rng(4)
    np.random.seed(4)
    x = np.sort(rng.uniform(size=60 if rep else 120))
    if rep:
        x = np.repeat(x, 2)
    X = x[:, None]
    sd = 0.05 + 0.5 * x ** 2
    Y = (np.sin(6 * x) + sd * rng.normal(size=len(x)))[:, None]
    layers = combine([kernel(length=np.array([0.5]), name='sexp', scale_est=True),
                      kernel(length=np.array([0.5]), name='sexp', scale_est=True)], [Hetero()])
    model = dgp(X, Y, layers, seed=2, vecchia=True, m=25)
    assert model.all_layer[0][0].vecch
    model.train(N=30, ess_burn=5, disable=True)
    assert model.all_layer[0][0].imp_NNarray is not None and model.all_layer[0][0].imp_NNarray.shape == (len(model.X), 26)
    mean_lat, logvar_lat = model.all_layer[0][0].output[:, 0], model.all_layer[0][1].output[:, 0]
    xs = model.X[:, 0]
    # one draw from the (Vecchia-approximate) conditional posterior: tight where the noise is small.  The reference's
    # approximation itself is coarse here (random ordering, later neighbours enter as observations): its posterior
    # mean is 0.06-0.09 rms away from the exact one on this design, so the bounds are looser than in the dense test.
    assert np.sqrt(np.mean((mean_lat - np.sin(6 * xs))[xs < 0.4] ** 2)) < 0.15
    assert np.sqrt(np.mean((mean_lat - np.sin(6 * xs)) ** 2)) < 0.45
    assert np.mean(logvar_lat[xs > 0.75]) > np.mean(logvar_lat[xs < 0.3]) + 1.0
    emu = emulator(model.estimate(), N=3, seed=5)
    xt = np.linspace(0.05, 0.95, 19)[:, None]
    mu, var = emu.predict(xt, m=25)
    lo = xt[:, 0] < 0.5
    assert mu.shape == (19, 1) and np.all(np.isfinite(mu)) and np.sqrt(np.mean((mu[lo, 0] - np.sin(6 * xt[lo, 0])) ** 2)) < 0.2
    assert var[xt[:, 0] > 0.75].mean() > 3 * var[xt[:, 0] < 0.3].mean()


@pytest.mark.parametrize('lik', ['Poisson', 'NegBin', 'ZIP', 'ZINB'])
def test_count_likelihood_dgp_end_to_end(eng, lik):
    """A DGP with a count likelihood on top (host plugin node, ESS on all latents, dgp.py:327-336,526-566 warm starts):
    the latent log-rate follows the truth and the emulator's predictive mean follows the rate."""
    import dgp_amd
    from dgp_amd import dgp, kernel, combine, emulator
    rng = np.random.default_rng(8)
    np.random.seed(8)
    x = np.sort(rng.uniform(size=70))
    X = np.repeat(x, 2)[:, None]
    rate = np.exp(1.0 + 1.2 * np.sin(5 * X[:, 0]))
    if lik in ('ZIP', 'ZINB'):
        base = rng.poisson(rate) if lik == 'ZIP' else rng.negative_binomial(5.0, 5.0 / (5.0 + rate))
        Y = (base * (rng.uniform(size=len(rate)) > 0.25))[:, None].astype(float)
    else:
        Y = (rng.poisson(rate) if lik == 'Poisson' else rng.negative_binomial(5.0, 5.0 / (5.0 + rate)))[:, None].astype(float)
    q = {'Poisson': 1, 'ZINB': 3}.get(lik, 2)
    layers = combine([kernel(length=np.array([0.5]), name='sexp', scale_est=True) for _ in range(q)], [getattr(dgp_amd, lik)()])
    model = dgp(X, Y, layers, seed=3)
    assert model.all_layer[1][0].rep is not None and model.all_layer[1][0].input.shape == (140, q)
    model.train(N=25, ess_burn=5, disable=True)
    lat = model.all_layer[0][0].output[:, 0]
    truth = 1.0 + 1.2 * np.sin(5 * model.X[:, 0])
    assert np.sqrt(np.mean((lat - truth) ** 2)) < {'Poisson': 0.45, 'ZINB': 1.0}.get(lik, 0.7)   # (one posterior draw; NegBin data are over-dispersed)
    emu = emulator(model.estimate(), N=3, seed=1)
    xt = np.linspace(0.05, 0.95, 15)[:, None]
    mu, var = emu.predict(xt)
    rt = np.exp(1.0 + 1.2 * np.sin(5 * xt[:, 0])) * (0.75 if lik in ('ZIP', 'ZINB') else 1.0)     # (a quarter structural zeros)
    assert mu.shape == (15, 1) and np.all(var[:, 0] > 0) and np.mean(np.abs(mu[:, 0] - rt) / rt) < (0.6 if lik in ('ZIP', 'ZINB') else 0.35)   # (140 counts hardly separate rate and inflation)
    assert np.all(var[:, 0] >= mu[:, 0] * 0.9)        # count noise: variance at least about the mean
    smp = emu.predict(xt, method='sampling', sample_size=50)
    assert smp[0].shape == (15, 150) and np.all(smp[0] >= 0)
    avg, per = emu.nllik(xt, rng.poisson(rt)[:, None].astype(float))
    assert np.isfinite(avg) and per.shape == (15,)


def test_not_positive_definite_raises_and_train_restarts(eng):
    """Error convention: a non-PD covariance surfaces as numpy.linalg.LinAlgError from the node methods, and
    dgp.train restarts from the last good hyper-parameters like the reference (dgp.py:1402-1412), at most three times."""
    from dgp_amd import dgp, kernel, combine
    rng = np.random.default_rng(2)
    X = rng.uniform(size=(30, 2))
    k = kernel(length=np.array([1.0]), nugget=0.0, name='sexp', engine=eng)
    k.input = np.concatenate((X, X[:3]))            # duplicated rows and no nugget: singular
    k.output = rng.normal(size=(33, 1))
    k.global_input, k.D = None, 2
    with pytest.raises(np.linalg.LinAlgError):
        k.log_likelihood_func()
    with pytest.raises(np.linalg.LinAlgError):
        k.llik(k.log_t())
    Y = np.sin(4 * X[:, :1]) + X[:, 1:]
    model = dgp(X, Y, combine([kernel(length=np.array([1.0]), name='sexp') for _ in range(2)],
                              [kernel(length=np.array([1.0]), name='sexp', scale_est=True)]), seed=5)
    model.train(N=2, ess_burn=2, disable=True)
    calls = {'n': 0}
    orig = model._m_step

    def flaky(**kw):   # (dgp.train passes early=True where the first round may be queued ahead of the host's refresh: dense models since round 6)
        calls['n'] += 1
        if calls['n'] == 2:
            raise np.linalg.LinAlgError('injected')
        return orig(**kw)
    model._m_step = flaky
    model.train(N=3, ess_burn=2, disable=True)
    assert model.N == 5 and calls['n'] == 2 + 3           # one failed attempt (2 calls) + a full rerun
    assert all(nd.para_path.shape[0] == 6 for layer in model.all_layer for nd in layer)
    model._m_step = lambda **kw: (_ for _ in ()).throw(np.linalg.LinAlgError('always'))
    with pytest.raises(RuntimeError):
        model.train(N=1, ess_burn=1, disable=True)


def test_gp_update_xy_and_metric(eng):
    """gp.update_xy / update_kernel (gp.py:144-209) and gp.metric ALM / MICE / VIGF (gp.py:271-324, functions.mice_var)
    against the oracle; emulator.to_vecchia / remove_vecchia switch the prediction mode."""
    from dgp_amd import gp, kernel, dgp, combine, emulator
    from oracle import dgp_oracle as O
    rng = np.random.default_rng(12)
    X = rng.uniform(size=(40, 2))
    f = lambda X: np.sin(5 * X[:, :1]) + X[:, 1:] ** 2
    k = kernel(length=np.array([0.6, 0.9]), name='matern2.5', scale_est=True, nugget=1e-4)
    model = gp(X[:30], f(X[:30]), k)
    model.train()
    length = k.length.copy()
    xc = rng.uniform(size=(25, 2))
    mu, s2 = model.predict(xc)
    assert np.array_equal(model.metric(xc, method='ALM', score_only=True), s2)
    mice = model.metric(xc, method='MICE', nugget_s=1.0, score_only=True)
    ref = s2 / O.mice_var(xc, xc, k.input_dim, k.connect, k.name, k.length, k.scale, k.nugget[0], 1.0).reshape(-1, 1)
    close(mice, ref, rtol=1e-8, atol=1e-12)
    idx, best = model.metric(xc, method='MICE')
    assert idx[0] == int(np.argmax(mice[:, 0])) and best[0] == mice[:, 0].max()
    vig = model.metric(xc, method='VIGF', score_only=True)
    near = np.argmin(((xc[:, None, :] - model.X[None]) ** 2).sum(-1), 1)
    close(vig, 4 * s2 * (mu - model.Y[near]) ** 2 + 2 * s2 ** 2, rtol=1e-12)
    # new data, hyper-parameters kept; then with replicates; then reset
    model.update_xy(X, f(X))
    assert model.n_data == 40 and k.input.shape == (40, 2) and np.array_equal(k.length, length) and k.rep is None
    mu2, _ = model.predict(X[30:])
    assert np.sqrt(np.mean((mu2 - f(X[30:])) ** 2)) < 0.05          # the ten new points are now interpolated
    Xr = np.concatenate((X, X[:7]))
    model.update_xy(Xr, f(Xr) + 0.01 * rng.normal(size=(47, 1)))
    assert model.n_data == 40 and k.rep is not None and len(k.rep) == 47 and k.W_diag.shape == (40,)
    model.update_xy(X, f(X), reset=True)
    assert np.array_equal(k.length, np.array([0.6, 0.9])) and k.rep is None
    # emulator mode switches
    d = dgp(X, f(X), combine([kernel(length=np.array([1.0]), name='sexp') for _ in range(2)],
                             [kernel(length=np.array([1.0]), name='sexp', scale_est=True, connect=np.arange(2))]), seed=1)
    d.train(N=3, ess_burn=3, disable=True)
    emu = emulator(d.estimate(), N=2, seed=2)
    a, _ = emu.predict(xc)
    emu.to_vecchia()
    b, _ = emu.predict(xc, m=39)            # all 40 points but the shortcut boundary: close to the dense prediction
    assert emu.vecch and np.sqrt(np.mean((a - b) ** 2)) < 0.05
    emu.remove_vecchia()
    c, _ = emu.predict(xc)
    close(c, a, rtol=1e-9, atol=1e-12)
    with pytest.raises(Exception):
        emu.remove_vecchia()


def test_prior_paths_and_summary(eng, capsys):
    """synthetic.path.generate (synthetic.py:20-46) against the oracle's fmvn with the same normals; utils.summary."""
    from dgp_amd import path, kernel, combine, summary, gp
    from oracle import dgp_oracle as O
    rng = np.random.default_rng(1)
    X = rng.uniform(size=(35, 2))
    layers = combine([kernel(length=np.array([0.5]), name='matern2.5', nugget=1e-6),
                      kernel(length=np.array([0.8]), name='sexp', scale=2.0, nugget=1e-5)],
                     [kernel(length=np.array([1.0]), name='matern2.5', scale=1.5, connect=np.arange(2), nugget=1e-6)])
    np.random.seed(11)
    got = path(X, layers).generate(2)
    assert got.shape == (1, 2, 35)
    np.random.seed(11)
    for i in range(2):
        x = X
        for layer in layers:
            out = np.empty((35, len(layer)))
            for k, nd in enumerate(layer):
                In = x if nd.connect is None else np.concatenate((x, X[:, nd.connect]), 1)
                cov = nd.scale[0] * O.k_matrix(In, nd.length, nd.nugget[0], nd.name)
                out[:, k] = O.fmvn(cov, np.random.normal(size=[35, 1]).ravel())
            x = out
        close(got[0, i], x[:, 0], rtol=1e-6, atol=1e-8)
    summary(layers[0][0])
    summary(gp(X, np.sin(X[:, :1]), kernel(length=np.array([1.0, 1.0]), scale_est=True)))
    txt = capsys.readouterr().out
    assert 'Matern-2.5' in txt and 'Squared-Exp' in txt and '(fixed)' in txt


@pytest.mark.parametrize('K', [2, 3])
def test_categorical_dgp_end_to_end(eng, K):
    """Classification DGP (Categorical likelihood: label encoding, +-2 sqrt(40) warm start, first sweeps with variance 40,
    ESS on all latents; emulator: latent moments aggregated over the imputations, then class probabilities)."""
    from dgp_amd import dgp, kernel, combine, emulator, Categorical, save_structure, load_structure
    rng = np.random.default_rng(6)
    np.random.seed(6)
    X = rng.uniform(size=(90, 2))
    score = np.sin(4 * X[:, 0]) + X[:, 1]
    names = np.array(['low', 'mid', 'top'])
    cls = (score > 0.9).astype(int) if K == 2 else np.digitize(score, [0.6, 1.2])
    Y = names[cls].reshape(-1, 1)
    q = 1 if K == 2 else K
    layers = combine([kernel(length=np.array([0.5]), name='sexp', scale_est=True) for _ in range(q)], [Categorical()])
    model = dgp(X, Y, layers, seed=2)
    lik = model.all_layer[1][0]
    assert lik.num_classes == K and lik.link == ('logit' if K == 2 else 'softmax') and set(np.unique(model.Y)) == set(range(K))
    assert all(nd.scale[0] != 40.0 for nd in model.all_layer[0])            # the start-up variance is restored
    model.train(N=15, ess_burn=5, disable=True)
    emu = emulator(model.estimate(), N=3, seed=4)
    xt = rng.uniform(size=(60, 2))
    st = np.sin(4 * xt[:, 0]) + xt[:, 1]
    truth = (st > 0.9).astype(int) if K == 2 else np.digitize(st, [0.6, 1.2])
    np.random.seed(1)
    p, pv = emu.predict(xt)
    assert p.shape == (60, 1 if K == 2 else K) and np.all((p >= 0) & (p <= 1)) and np.all(pv >= 0)
    pred = (p[:, 0] > 0.5).astype(int) if K == 2 else np.argmax(p, 1)
    assert np.mean(pred == truth) > 0.8
    if K > 2:
        assert np.allclose(p.sum(1), 1.0, atol=1e-9)
    smp = emu.predict(xt[:7], method='sampling', sample_size=20)
    assert len(smp) == (1 if K == 2 else K) and smp[0].shape == (7, 60)
    # a label outside [0, num_classes) never reaches the device log-density (it indexes the latent columns by the label)
    keep = lik.output
    lik.output = keep.astype(float).copy()
    lik.output[3, 0] = K
    with pytest.raises(ValueError, match='class labels'):
        model.imp.sample(burnin=1)
    lik.output = keep
    model.imp.sample(burnin=1)
    avg, per = emu.nllik(xt, truth.reshape(-1, 1).astype(float if K == 2 else int))
    assert np.isfinite(avg) and per.shape == (60,) and np.all(per >= 0)     # (few iterations: confident latents, so a few
    import os, tempfile                                                    #  misclassified points dominate the average)
    with tempfile.TemporaryDirectory() as tmp:
        save_structure(model.estimate(), os.path.join(tmp, 'c'))
        back = load_structure(os.path.join(tmp, 'c'))
        assert back[1][0].name == 'Categorical' and back[1][0].num_classes == K and list(back[1][0].class_encoder.classes_) == list(names[:K])
    Xn = rng.uniform(size=(40, 2))
    sn = np.sin(4 * Xn[:, 0]) + Xn[:, 1]
    model.update_xy(Xn, names[(sn > 0.9).astype(int) if K == 2 else np.digitize(sn, [0.6, 1.2])].reshape(-1, 1))
    assert model.n_data == 40 and set(np.unique(model.Y)) <= set(range(K))


def test_reference_prior_in_the_ess_target(eng):
    """A second-layer node with prior_name='ref': the ESS target carries the prior term with its input-dependent scaling
    constant (kernel_class.py:489-491); checked against the oracle for one candidate block, then a short training run."""
    from dgp_amd import dgp, kernel, combine
    from dgp_amd.imputation import imputer
    from oracle import dgp_oracle as O
    rng = np.random.default_rng(9)
    X = rng.uniform(size=(40, 2))
    Y = np.sin(4 * X[:, :1]) * X[:, 1:]
    layers = combine([kernel(length=np.array([1.0]), name='sexp') for _ in range(2)],
                     [kernel(length=np.array([0.8, 1.1]), name='matern2.5', scale_est=True, prior_name='ref', nugget=1e-3)])
    model = dgp(X, Y, layers, seed=4)
    imp, nd = model.imp, model.all_layer[1][0]
    imp._attach()
    F = imp.F[0]
    ll, info = imp._upper_loglik(0, F[None])
    Fh = F.cpu().numpy()
    base = O.log_likelihood(Fh[:, nd.input_dim], nd.output, nd.length, nd.scale, nd.nugget[0], nd.name)
    cl = (Fh.max(0) - Fh.min(0)) / 40 ** (1 / 2)
    t = np.sum(cl / nd.length) + nd.nugget[0]
    close(ll[0], float(np.ravel(base)[0]) + nd.prior_coef[0] * np.log(t) - nd.prior_coef[1] * t, rtol=1e-9)
    model.train(N=3, ess_burn=2, disable=True)
    assert np.all(np.isfinite(nd.para_path)) and nd.para_path.shape[0] == 4


def test_small_api_pieces(eng, tmp_path):
    """path.k_matrix, kernel.gfod, dgp.plot (headless), the p* entry points with their pool arguments, lgp.temp_all_layer."""
    import matplotlib
    matplotlib.use('Agg')
    from dgp_amd import dgp, kernel, combine, emulator, path, gp
    from oracle import dgp_oracle as O
    rng = np.random.default_rng(3)
    X = rng.uniform(size=(30, 2))
    for name in ('sexp', 'matern2.5'):
        K = path.k_matrix(X, np.array([0.4, 0.9]), name)
        Kr = O.corr_matrix(X, np.array([0.4, 0.9]), name)
        np.fill_diagonal(Kr, 1.0)
        close(K, Kr, rtol=1e-12, atol=1e-14)
    k = kernel(length=np.array([0.5]), name='sexp', prior_name='ga', prior_coef=np.array([1.6, 0.3]))
    close(k.gfod(np.array([2.0])), [k.prior_coef[0] - k.prior_coef[1] * 2.0])
    k = kernel(length=np.array([0.5]), name='sexp', prior_name='inv_ga', prior_coef=np.array([1.6, 0.3]))
    close(k.gfod(np.array([2.0])), [-k.prior_coef[0] + k.prior_coef[1] / 2.0])
    Y = np.sin(5 * X[:, [0]]) + X[:, [1]]
    model = dgp(X, Y, combine([kernel(length=np.array([1.0]), name='sexp') for _ in range(2)],
                              [kernel(length=np.array([1.0]), name='sexp', scale_est=True)]), seed=1)
    model.ptrain(N=3, ess_burn=2, disable=True, core_num=2)
    model.plot(1, 1)
    model.plot(2, 1, width=3., height=0.8)
    emu = emulator(model.estimate(), N=2)
    xt = rng.uniform(size=(7, 2))
    a = emu.ppredict(xt, chunk_num=3, core_num=2)
    b = emu.predict(xt)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(emu.ploo(X, core_num=2)[0], emu.loo(X)[0])
    assert np.array_equal(emu.pmetric(xt, method='ALM', score_only=True, chunk_num=2, core_num=2), emu.metric(xt, method='ALM', score_only=True))
    g = gp(X, Y, kernel(length=np.array([0.5, 0.5]), name='matern2.5', scale_est=True, nugget_est=True))
    g.train()
    assert np.array_equal(g.ppredict(xt, chunk_num=2, core_num=2)[0], g.predict(xt)[0])
    assert np.array_equal(g.pmetric(xt, method='MICE', score_only=True, core_num=2), g.metric(xt, method='MICE', score_only=True))


def test_compute_stats_falls_back_to_the_pseudo_inverse(eng):
    """kernel.compute_stats on an indefinite R (a repeated input row and a slightly negative nugget, so that no rounding
    decides which branch runs): the factorisation fails and the pseudo-inverse takes over as in kernel_class.py:745-751; R^-1, R^-1 y and the predictions agree with scipy's pinvh
    on the oracle's R.  The emulator's per-imputation statistics take the same route."""
    from scipy.linalg import pinvh
    from dgp_amd import kernel, emulator
    from oracle import dgp_oracle as O
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
    R = O.corr_matrix(X, nd.length, 'matern2.5')
    R[np.arange(n), np.arange(n)] = 1.0 - 1e-3
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.cholesky(R)
    Rinv = pinvh(R, check_finite=False)
    close(nd.Rinv, Rinv, rtol=1e-7, atol=1e-7 * np.abs(Rinv).max())
    close(nd.Rinv_y, Rinv @ y, rtol=1e-7, atol=1e-7 * np.abs(Rinv @ y).max())
    xt = rng.uniform(size=(9, 2))
    m, v = nd.gp_prediction(xt, None)
    mr, vr = O.gp_predict(xt, X, Rinv, Rinv @ y, 1.7, nd.length, -1e-3, 'matern2.5')
    close(m, mr, rtol=1e-6, atol=1e-8)
    close(v, vr, rtol=1e-5, atol=1e-7)
    emu = emulator([[nd]], N=1)
    mu, var = emu.predict(xt)
    close(mu[:, 0], mr, rtol=1e-6, atol=1e-8)


@pytest.mark.parametrize('block', [True, False])
def test_ess_stationary_distribution_is_the_analytic_posterior(eng, block):
    """long-run mean and covariance of a one-node latent layer under a Gaussian likelihood plugged in
    through the likelihood-node protocol (llik on .input, likelihood_class.py:30-90) against the conjugate posterior
    N(K (K + s^2 I)^-1 y,  K - K (K + s^2 I)^-1 K).  Statistical tolerance: 4000 kept sweeps, thinned by 5."""
    from dgp_amd import kernel
    from dgp_amd.imputation import imputer, DrawStream
    from oracle import dgp_oracle as O

    class Gauss:
        type, name, rep, exact_post_idx = 'likelihood', 'Gauss', None, None

        def __init__(self, s2):
            self.s2, self.input_dim = s2, np.array([0])

        def llik(self):
            return -0.5 * np.sum((self.output - self.input) ** 2) / self.s2

    rng = np.random.default_rng(4)
    n, s2, scale = 6, 0.3, 1.4
    X = np.sort(rng.uniform(size=(n, 1)), 0)
    y = np.sin(5 * X) + rng.normal(size=(n, 1)) * np.sqrt(s2)
    nd = kernel(length=np.array([0.4]), scale=scale, nugget=1e-8, name='matern2.5', input_dim=np.array([0]), engine=eng)
    nd.input, nd.output, nd.global_input, nd.vecch, nd.D = X, np.zeros((n, 1)), None, False, 1
    lik = Gauss(s2)
    lik.input, lik.output = nd.output.copy(), y
    imp = imputer([[nd], [lik]], block=block, draws=DrawStream(seed=11), engine=eng, batch=4)
    imp.sample(burnin=200)
    keep = []
    for _ in range(4000):
        imp.sample(burnin=5)
        keep.append(nd.output[:, 0].copy())
    F = np.asarray(keep)
    K = scale * O.corr_matrix(X, nd.length, 'matern2.5')
    K[np.arange(n), np.arange(n)] = scale * (1.0 + 1e-8)
    G = K @ np.linalg.inv(K + s2 * np.eye(n))
    mean, cov = (G @ y)[:, 0], K - G @ K
    sd = np.sqrt(np.diag(cov))
    # Monte-Carlo error of a mean of 4000 (mildly autocorrelated) draws ~ sd / sqrt(2000); 5 sigma
    assert np.all(np.abs(F.mean(0) - mean) < 5 * sd / np.sqrt(2000)), (F.mean(0), mean)
    emp = np.cov(F.T)
    assert np.all(np.abs(emp - cov) < 0.12 * np.sqrt(np.outer(np.diag(cov), np.diag(cov)))), (emp, cov)
    assert np.allclose(lik.input[:, 0], nd.output[:, 0])


def test_emulator_points_sharding_two_ranks(tmp_path):
    """emulator(shard='points') on two processes (gloo rendezvous, both on this GPU): every rank holds the same
    imputations and predicts its block of test points; the gathered result equals the single-process prediction, and
    the imputation-sharded emulator (shard=True) of the same run reduces to one consistent answer on both ranks."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / 'worker.py'
    script.write_text("""
import os, sys
sys.path.insert(0, %r)
import numpy as np
from dgp_amd import dgp, kernel, combine, emulator, dist as dd
dd.init_from_env('gloo')
rng = np.random.default_rng(1)
X = rng.uniform(size=(60, 2)); Y = np.sin(5 * X[:, [0]]) + X[:, [1]] ** 2
layers = combine([kernel(length=np.array([1.0]), name='matern2.5') for _ in range(2)],
                 [kernel(length=np.array([1.0]), name='matern2.5', scale_est=True, connect=np.arange(2))])
model = dgp(X, Y, layers, seed=5)
model.train(N=4, ess_burn=3, disable=True)
est = model.estimate()
xt = rng.uniform(size=(37, 2))
import copy
ref = emulator(copy.deepcopy(est), N=4, seed=9, shard=False).predict(xt)
emu = emulator(copy.deepcopy(est), N=4, seed=9, shard='points')
assert emu.N == 4 and emu.shard_points
mu, var = emu.predict(xt)
np.testing.assert_allclose(mu, ref[0], rtol=1e-10, atol=1e-12)
np.testing.assert_allclose(var, ref[1], rtol=1e-9, atol=1e-13)
ml, vl = emu.predict(xt, full_layer=True)
np.testing.assert_allclose(ml[-1], ref[0], rtol=1e-10, atol=1e-12)
assert ml[0].shape == (37, 2)
one = emu.predict(xt[:1])                      # fewer rows than ranks
np.testing.assert_allclose(one[0], ref[0][:1], rtol=1e-10, atol=1e-12)
sh = emulator(copy.deepcopy(est), N=4, seed=9)  # imputations sharded: 2 per rank, one all-reduce
assert sh.shard and sh.N == 2
ms, vs = sh.predict(xt)
box = [ms if dd.rank() == 0 else None]
dd.td.broadcast_object_list(box, src=0)
assert np.array_equal(box[0], ms)               # both ranks hold the reduced moments
assert np.sqrt(np.mean((ms - ref[0]) ** 2)) < 0.1
dd.barrier()
print('rank', dd.rank(), 'ok')
""" % root)
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT='29547', WORLD_SIZE='2')
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r), LOCAL_RANK='0'),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(2)]
    outs = [p.communicate(timeout=600)[0].decode() for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o
        assert 'ok' in o


@pytest.mark.parametrize('lik', ['Poisson', 'Categorical'])
def test_emulator_loo_under_a_likelihood_layer(eng, lik):
    """Dense leave-one-out with a likelihood node on top (emulation.py:109-143, :711-716 for Categorical): the downdate
    walk feeds the same likelihood post-processing as the reference's re-conditioning route and agrees with it."""
    from dgp_amd import dgp, kernel, combine, emulator, Poisson, Categorical
    rng = np.random.default_rng(6)
    n = 50
    X = rng.uniform(size=(n, 2))
    # (Matern with a 1e-4 nugget: the two routes differ by rounding x cond(R) x scale, kept small here)
    K = lambda **kw: kernel(length=np.array([1.0]), name='matern2.5', nugget=1e-4, **kw)
    if lik == 'Poisson':
        Y = rng.poisson(np.exp(1 + np.sin(4 * X[:, [0]]))).astype(float)
        layers = combine([K() for _ in range(2)], [K(scale_est=True)], [Poisson()])
    else:
        Y = (X[:, [0]] + 0.3 * np.sin(6 * X[:, [1]]) > 0.55).astype(int)
        layers = combine([K() for _ in range(2)], [K(scale_est=True)], [Categorical(num_classes=2)])
    model = dgp(X, Y, layers, seed=4)
    model.train(N=5, ess_burn=3, disable=True)
    emu = emulator(model.estimate(), N=3, seed=2)
    mu, var = emu.loo(X)
    gps = [nd for layer in emu.all_layer for nd in layer if nd.type == 'gp']
    for nd in gps:
        nd.loo_state, nd.vecch = True, True
    try:
        mu_ref, var_ref = emu._aggregate(emu._layer_moments(X, 'vecchia', n))
    finally:
        for nd in gps:
            nd.loo_state, nd.vecch = False, False
    assert mu.shape == mu_ref.shape and mu.shape[0] == n
    close(mu, mu_ref, rtol=1e-4, atol=1e-6)
    close(var, var_ref, rtol=1e-3, atol=1e-6)
    assert np.all(np.isfinite(mu)) and np.all(var >= 0)
    if lik == 'Categorical':
        assert np.all(mu >= 0) and np.all(mu <= 1)


@pytest.mark.parametrize('nout', [1, 3])
@pytest.mark.parametrize('batch', [12, 2])
def test_queued_ess_equals_host_loop(eng, nout, batch):
    """imputer.sample on a two-layer model: the device-resident accept / shrink loop (dgpamd_ess_queue, zero host round trips
    inside the I-step) takes the same decisions as the host loop -- same latents, same number of proposals, the
    uniform stream left at the same position -- with one and with several GP nodes in the layer above (their
    log-likelihoods are summed, imputation.py:91-106); batch=2 forces updates that run out of queued batches: with
    the one hidden layer here the next queue continues them on the device."""
    from dgp_amd import dgp, kernel, combine
    rng = np.random.default_rng(5)
    n, d = 300, 3
    X = rng.uniform(size=(n, d))
    Y = np.stack([np.sin(3 * X[:, 0] + k) + X[:, 1] ** 2 * (k + 1) for k in range(nout)], 1)
    Y = (Y - Y.mean(0)) / Y.std(0)

    def run(queued):
        layers = combine([kernel(length=np.array([1.0]), name='matern2.5') for _ in range(d)],
                         [kernel(length=np.array([0.8]), name='matern2.5' if k % 2 == 0 else 'sexp', scale_est=True, connect=np.arange(d))
                          for k in range(nout)])
        model = dgp(X, Y, layers, seed=3)
        model.imp.batch = batch
        model.imp.batch_next = min(4, batch)
        model.imp.queued = queued
        for _ in range(2):
            model.imp.sample(burnin=6)
        F = np.stack([nd.output[:, 0] for nd in model.all_layer[0]], 1)
        return F, dict(model.imp.stats), model.imp.draws.uniform_peek(3)

    Fq, sq, uq = run(True)
    Fh, sh, uh = run(False)
    close(Fq, Fh, rtol=1e-9, atol=1e-11)
    assert sq == sh, (sq, sh)   # proposals, updates, batches
    assert uq == uh


@pytest.mark.parametrize('nout', [1, 3])
def test_queued_open_update_policies_agree(eng, nout, monkeypatch):
    """The two ways an update that ran out of queued batches is carried on in a model with one hidden layer -- the next queue
    continues it on the device (the default), or the host loop finishes it and the rest is queued anew (DGPAMD_ESS_RESUME=0,
    read per call) -- take the same decisions: same latents, same counts, the uniform stream left at the same position.
    Batches of 2, two queued per update: most updates are left open at least once."""
    from dgp_amd import dgp, kernel, combine
    rng = np.random.default_rng(5)
    n, d = 300, 3
    X = rng.uniform(size=(n, d))
    Y = np.stack([np.sin(3 * X[:, 0] + k) + X[:, 1] ** 2 * (k + 1) for k in range(nout)], 1)
    Y = (Y - Y.mean(0)) / Y.std(0)

    def run(resume):
        if resume:
            monkeypatch.delenv('DGPAMD_ESS_RESUME', raising=False)
        else:
            monkeypatch.setenv('DGPAMD_ESS_RESUME', '0')
        layers = combine([kernel(length=np.array([1.0]), name='matern2.5') for _ in range(d)],
                         [kernel(length=np.array([0.8]), name='matern2.5' if k % 2 == 0 else 'sexp', scale_est=True, connect=np.arange(d))
                          for k in range(nout)])
        model = dgp(X, Y, layers, seed=3)
        model.imp.batch = model.imp.batch_next = 2
        before = model.imp.queued_calls
        for _ in range(2):
            model.imp.sample(burnin=6)
        F = np.stack([nd.output[:, 0] for nd in model.all_layer[0]], 1)
        return F, dict(model.imp.stats), model.imp.draws.uniform_peek(3), model.imp.queued_calls - before

    Fd, sd, ud, qd = run(True)
    Fh, sh, uh, qh = run(False)
    print('stats: device resume', sd, 'host finish', sh, 'queued calls', qd, qh)
    close(Fd, Fh, rtol=1e-9, atol=1e-11)
    assert sd == sh, (sd, sh)   # proposals, updates, batches
    assert ud == uh
    assert qd == 2 and qh == 2


@pytest.mark.parametrize('shape', ['vecchia_top', 'vecchia_all', 'three_layers', 'three_layers_vecchia'])
@pytest.mark.parametrize('batch', [12, 2])
def test_queued_ess_equals_host_loop_other_shapes(eng, shape, batch):
    """The device-resident accept / shrink loop for the model shapes round 2 left to the host loop:
    a Vecchia node upstairs (kernel_class.py:494-509: every speculative batch gathers the candidates' ordered inputs and
    runs vecchia_llik for all of them in one row launch), Vecchia in both layers (sparse prior draws ahead), and three
    layers (imputation.py:22-42: per sweep and hidden layer the prior draw from the CURRENT inputs -- K assembly,
    factorisation, triangular product queued on the device as well -- then one queued update; one fetch per I-step).
    Same latents in every layer, same proposal / batch / update counts, the uniform stream left at the same position as
    the host loop; batch=2 forces updates that run out of queued batches: with one hidden layer they are continued by the
    next queue, with several they are finished by the host loop."""
    from dgp_amd import dgp, kernel, combine
    rng = np.random.default_rng(11)
    n, d = 260, 3
    X = rng.uniform(size=(n, d))
    Y = (np.sin(3 * X[:, :1]) + X[:, 1:2] ** 2)
    Y = (Y - Y.mean(0)) / Y.std(0)
    deep = shape.startswith('three')

    def run(queued):
        np.random.seed(7)   # (the Vecchia orderings are numpy.random.permutation draws, kernel_class.py:255: the same in both runs)
        ls = [[kernel(length=np.array([1.0]), name='matern2.5') for _ in range(d)]]
        if deep:
            ls.append([kernel(length=np.array([1.2]), name='sexp' if k else 'matern2.5', connect=np.arange(d)) for k in range(2)])
        ls.append([kernel(length=np.array([0.8]), name='matern2.5', scale_est=True, connect=np.arange(d))])
        vecchia = shape in ('vecchia_all', 'three_layers_vecchia')
        model = dgp(X, Y, combine(*ls), seed=3, vecchia=vecchia, m=12)
        if shape == 'vecchia_top':   # dense hidden layer, Vecchia node upstairs
            top = model.all_layer[-1][0]
            top.vecch, top.m = True, 12
            model.imp.update_ord_nn()
        model.imp.batch = batch
        model.imp.batch_next = min(4, batch)
        model.imp._batch_default = False   # (keep these sizes in the queue too: the batch counts are compared below)
        model.imp.queued = queued
        for _ in range(2):
            model.imp.sample(burnin=4)
        F = [np.stack([nd.output[:, 0] for nd in layer], 1) for layer in model.all_layer[:-1]]
        return F, dict(model.imp.stats), model.imp.draws.uniform_peek(3)

    Fq, sq, uq = run(True)
    Fh, sh, uh = run(False)
    for a, b in zip(Fq, Fh):
        close(a, b, rtol=1e-9, atol=1e-11)
    assert sq == sh, (sq, sh)   # proposals, updates, batches
    assert uq == uh


@pytest.mark.parametrize('bad_layer', [0, 1])
def test_queued_deep_reports_a_failed_prior_factor(eng, bad_layer):
    """A prior covariance that is not positive definite must stop the device queue exactly as it stops the host loop and
    the reference (imputation.py:54-63 -> numpy's cholesky raises; dgp.train restarts on it): LinAlgError, whichever
    operation of a fetch window the factorisation belongs to.  ADVICE r03: the FIRST operation of a window noted its info
    word in the shared device state and the queue's fresh reset then wiped it -- the sampler carried on with nu from a
    failed factor.  Three layers under an injected normal stream, so that layer 0's prior is factored inside the window
    too (bad_layer = 0: the window's first operation; 1: a later one)."""
    from dgp_amd import dgp, kernel, combine
    from dgp_amd.imputation import DrawStream
    rng = np.random.default_rng(11)
    n, d = 200, 3
    X = rng.uniform(size=(n, d))
    Y = (np.sin(3 * X[:, :1]) + X[:, 1:2] ** 2)
    Y = (Y - Y.mean(0)) / Y.std(0)
    for queued in (True, False):
        ls = [[kernel(length=np.array([1.0]), name='matern2.5') for _ in range(d)],
              [kernel(length=np.array([1.2]), name='sexp' if k else 'matern2.5', connect=np.arange(d)) for k in range(2)],
              [kernel(length=np.array([0.8]), name='matern2.5', scale_est=True, connect=np.arange(d))]]
        model = dgp(X, Y, combine(*ls), seed=3)
        model.imp.queued = queued
        before = model.imp.queued_calls
        model.imp.sample(burnin=1)   # (a healthy call first: plans and buffers exist)
        assert model.imp.queued_calls - before == (1 if queued else 0)   # (the shape does run through the device queue)
        zr = np.random.default_rng(5)
        model.imp.draws = DrawStream(seed=9, z=[zr.normal(size=n) for _ in range(64)])
        model.all_layer[bad_layer][0].nugget = np.array([-2.0])   # K + nugget I with a negative diagonal
        model.imp._factor_cache = {}
        with pytest.raises(np.linalg.LinAlgError):
            model.imp.sample(burnin=2)


@pytest.mark.parametrize('lik', ['Poisson', 'NegBin', 'ZIP', 'ZINB', 'logit', 'probit', 'softmax', 'robustmax'])
@pytest.mark.parametrize('batch', [12, 2])
def test_queued_ess_equals_host_loop_likelihood_tops(eng, lik, batch):
    """The device-resident accept / shrink loop with a likelihood node on top (imputation.py:71-78,
    91-106 -> <likelihood>.llik()): the node's summed log-density is a library kernel (dgpamd_lik_loglik) that the host
    loop and the queue both use, so the two take the same decisions -- same latents in every layer, same proposal /
    batch / update counts, the uniform stream left at the same position.  Count data with replicates for NegBin.  batch=2
    forces updates that run out of queued batches: two hidden layers here, so the host loop finishes them."""
    from dgp_amd import dgp, kernel, combine, Poisson, NegBin, ZIP, ZINB, Categorical
    rng = np.random.default_rng(23)
    n, d = 180, 2
    X = rng.uniform(size=(n, d))
    if lik == 'NegBin':   # replicated sites
        X = np.concatenate((X[:120], X[:60]))
    eta = 1.2 + np.sin(4 * X[:, 0]) + X[:, 1]
    if lik in ('Poisson', 'NegBin', 'ZIP', 'ZINB'):
        Y = rng.poisson(np.exp(eta)).astype(float)[:, None]
        if lik in ('ZIP', 'ZINB'):
            Y[rng.uniform(size=n) < 0.25] = 0.0
        top = {'Poisson': Poisson, 'NegBin': NegBin, 'ZIP': ZIP, 'ZINB': ZINB}[lik]()
        nlat = {'Poisson': 1, 'NegBin': 2, 'ZIP': 2, 'ZINB': 3}[lik]
    elif lik in ('logit', 'probit'):
        Y = (eta > 2.2).astype(int)[:, None]
        top, nlat = Categorical(num_classes=2, link=lik), 1
    else:
        Y = np.digitize(eta, [1.8, 2.6])[:, None]
        top, nlat = Categorical(num_classes=3, link=lik), 3

    def run(queued):
        np.random.seed(7)   # (warm starts that draw from numpy's global stream: the same in both runs)
        layers = combine([kernel(length=np.array([1.0]), name='matern2.5') for _ in range(d)],
                         [kernel(length=np.array([0.9]), name='sexp' if k % 2 else 'matern2.5', scale_est=True, connect=np.arange(d))
                          for k in range(nlat)], [top])
        model = dgp(X, Y, layers, seed=3)
        model.imp.batch = batch
        model.imp.batch_next = min(4, batch)
        model.imp._batch_default = False
        model.imp.queued = queued
        for _ in range(2):
            model.imp.sample(burnin=4)
        F = [np.stack([nd.output[:, 0] for nd in layer], 1) for layer in model.all_layer[:-1]]
        return F, dict(model.imp.stats), model.imp.draws.uniform_peek(3)

    Fq, sq, uq = run(True)
    Fh, sh, uh = run(False)
    for a, b in zip(Fq, Fh):
        assert np.all(np.isfinite(a))
        close(a, b, rtol=1e-9, atol=1e-11)
    assert sq == sh, (sq, sh)
    assert uq == uh
    assert sq['updates'] > 0 and sq['batches'] >= sq['updates']


def test_queued_ess_equals_host_loop_vecchia_under_a_likelihood(eng):
    """Vecchia GP layers with a count likelihood on top: the queue's three ingredients at once -- sparse prior draws by the
    level schedule, a Vecchia node upstairs of the first layer, the library's log-density upstairs of the second -- against
    the host loop: same latents, same counts, same position in the uniform stream."""
    from dgp_amd import dgp, kernel, combine, Poisson
    rng = np.random.default_rng(29)
    n, d = 240, 2
    X = rng.uniform(size=(n, d))
    Y = rng.poisson(np.exp(1.0 + np.sin(4 * X[:, 0]) + X[:, 1])).astype(float)[:, None]

    def run(queued):
        np.random.seed(7)
        layers = combine([kernel(length=np.array([1.0]), name='matern2.5') for _ in range(d)],
                         [kernel(length=np.array([0.9]), name='sexp', scale_est=True, connect=np.arange(d))], [Poisson()])
        model = dgp(X, Y, layers, seed=3, vecchia=True, m=10)
        model.imp.batch, model.imp.batch_next, model.imp._batch_default, model.imp.queued = 6, 3, False, queued
        for _ in range(2):
            model.imp.sample(burnin=3)
        F = [np.stack([nd.output[:, 0] for nd in layer], 1) for layer in model.all_layer[:-1]]
        return F, dict(model.imp.stats), model.imp.draws.uniform_peek(3)

    Fq, sq, uq = run(True)
    Fh, sh, uh = run(False)
    for a, b in zip(Fq, Fh):
        assert np.all(np.isfinite(a))
        close(a, b, rtol=1e-9, atol=1e-11)
    assert sq == sh and uq == uh, (sq, sh)


def test_mice_var_ghdiag_nllik_match_reference(eng, golden):
    """functions.mice_var / ghdiag (functions.py:233-256) and emulator.nllik (emulation.py:856-914) against values recorded
    from the reference (g22, g23): the smoothed candidate-set variance behind metric('MICE'), the Gauss-Hermite predictive
    likelihood, and the whole negative predicted log-likelihood of a Poisson-likelihood DGP from the reference's imputations."""
    from dgp_amd import kernel, Poisson, Hetero
    from dgp_amd.emulation import emulator, _mice_var
    from dgp_amd.likelihood_class import ghdiag
    g = golden('g22_mice_ghdiag')
    for i in range(2):
        glob = bool(g['m%d_glob' % i])
        nd = kernel(length=g['m%d_length' % i].copy(), scale=1.7, nugget=1e-6, name=str(g['m%d_name' % i]), input_dim=np.arange(3),
                    connect=np.arange(2) if glob else None, engine=eng)
        s2 = _mice_var(eng, g['m%d_x' % i], g['m%d_xe' % i], nd, 1e-3)
        close(s2, g['m%d_sigma2' % i].ravel(), rtol=1e-8)
    close(ghdiag(Poisson(input_dim=np.array([0])).pllik, g['gh_mu'], g['gh_var'], g['gh_y']), g['gh_poisson'], rtol=1e-12)
    close(ghdiag(Hetero(input_dim=np.array([0, 1])).pllik, g['gh_mu2'], g['gh_var2'], g['gh_y2']), g['gh_hetero'], rtol=1e-12)
    d = golden('g23_nllik_poisson')
    S = int(d['n_imp'])
    est = build_structure(d, 's0_', eng) + [[Poisson(input_dim=np.array([0]))]]
    emu = emulator.__new__(emulator)
    emu.all_layer, emu.n_layer, emu.vecch, emu.engine = est, len(est), False, eng
    emu.N = emu.N_total = S
    emu.shard = False
    emu.latents = []
    for s_ in range(S):
        ls = build_structure(d, 's%d_' % s_, eng)
        emu.latents.append([np.stack([nd.output[:, 0] for nd in layer], 1) for layer in ls])
    emu.orders = []
    emu._stats = None
    avg, per = emu.nllik(d['xt'], d['yt'])
    close(per, d['per'], rtol=1e-6, atol=1e-9)
    close(avg, d['avg'], rtol=1e-6)


def test_lockstep_mstep_equals_per_node_maximise(eng):
    """dgp._m_step drives scipy's L-BFGS-B core for all nodes in lock-step with batched device objectives
    (dgp_amd.mstep, dgpamd_llik_batch); kernel.maximise() runs scipy.optimize.minimize on one node at a time like the
    reference (kernel_class.py:516-579, dgp.py:1391-1398).  On two identical copies of a model both leave the SAME
    para_path rows and hyper-parameters, bit for bit (same iterates, same objective values)."""
    from dgp_amd import dgp, kernel, combine
    rng = np.random.default_rng(12)
    n, d = 200, 3
    X = rng.uniform(size=(n, d))
    f = np.sin(1.0 / ((0.7 * X[:, 0] + 0.3) * (0.7 * X[:, 1] + 0.3))) + 0.5 * X[:, 2] ** 2
    Y = ((f - f.mean()) / f.std())[:, None]

    def build():
        layers = combine([kernel(length=np.array([1.0]), name='matern2.5') for _ in range(d)],
                         [kernel(length=np.array([1.0, 0.8, 1.2, 1.0, 0.9, 1.1]), name='matern2.5', scale_est=True, nugget_est=True,
                                 connect=np.arange(d))])
        m = dgp(X, Y, layers, seed=4)
        m.imp.sample(burnin=3)
        return m

    a, b = build(), build()
    a._m_step()                                   # lock-step, batched
    for l, layer in enumerate(b.all_layer):       # one node after another
        for nd in layer:
            nd.engine = b.engine
            if l != 0:
                nd.r2()
            nd.maximise()
    for la, lb in zip(a.all_layer, b.all_layer):
        for na, nb in zip(la, lb):
            assert np.array_equal(na.para_path, nb.para_path), (na.para_path[-1], nb.para_path[-1])
            assert np.array_equal(na.length, nb.length) and np.array_equal(na.scale, nb.scale) and np.array_equal(na.nugget, nb.nugget)


def test_lockstep_vecchia_mstep_equals_per_node_maximise(eng):
    """The Vecchia nodes of a layer are fitted in lock-step too (dgp_amd.mstep.maximise_lockstep_vecch: every round's
    vecchia_nllik evaluations queued back to back, one fetch); kernel.maximise() fits one node at a time like the
    reference (kernel_class.py:516-579 with llik_vecch).  Same para_path rows and hyper-parameters, bit for bit."""
    from dgp_amd import dgp, kernel, combine
    rng = np.random.default_rng(21)
    n, d = 500, 3
    X = rng.uniform(size=(n, d))
    f = np.sin(4 * X[:, 0]) * np.cos(3 * X[:, 1]) + 0.5 * X[:, 2]
    Y = ((f - f.mean()) / f.std())[:, None]

    def build():
        np.random.seed(9)
        layers = combine([kernel(length=np.array([1.0]), name='matern2.5') for _ in range(d)],
                         [kernel(length=np.array([1.0]), name='sexp', scale_est=True, nugget_est=True, connect=np.arange(d))])
        m = dgp(X, Y, layers, vecchia=True, m=12, seed=4)
        m.imp.sample(burnin=2)
        return m

    a, b = build(), build()
    for la, lb in zip(a.all_layer, b.all_layer):
        for na, nb in zip(la, lb):
            assert np.array_equal(na.output, nb.output) and np.array_equal(na.input, nb.input)
    a._m_step()                                   # lock-step over the Vecchia nodes of each layer
    for l, layer in enumerate(b.all_layer):       # one node after another
        for nd in layer:
            nd.engine = b.engine
            if l != 0:
                nd.r2()
            nd.maximise()
    for la, lb in zip(a.all_layer, b.all_layer):
        for na, nb in zip(la, lb):
            assert na.para_path.shape[0] == 2
            assert np.array_equal(na.para_path, nb.para_path), (na.para_path[-1], nb.para_path[-1])
            assert np.array_equal(na.length, nb.length) and np.array_equal(na.scale, nb.scale) and np.array_equal(na.nugget, nb.nugget)


def test_vecchia_training_does_not_depend_on_the_host_overlaps(eng, monkeypatch):
    """dgp.train on a Vecchia model queues the M-step's first evaluations from the imputer's device state while the latents
    are still travelling to the host (imputer.sample(detach=False), dgp._mstep_can_start_early) and keeps two groups of
    optimisers in flight (mstep.minimize_lockstep(groups=2)).  Both are schedules, not algorithms: hyper-parameters, paths,
    latents, node inputs and neighbour arrays after five iterations (refreshes at 2 and 4) equal the plain order's, bit for bit."""
    from dgp_amd import dgp, kernel, combine
    rng = np.random.default_rng(33)
    n, d = 600, 4
    X = rng.uniform(size=(n, d))
    f = np.sin(4 * X[:, 0]) * np.cos(3 * X[:, 1]) + 0.5 * X[:, 2] - X[:, 3] ** 2
    Y = ((f - f.mean()) / f.std())[:, None]

    def run(early, groups):
        monkeypatch.setenv('DGPAMD_MSTEP_EARLY', early)
        monkeypatch.setenv('DGPAMD_MSTEP_GROUPS', groups)
        np.random.seed(3)
        layers = combine([kernel(length=np.array([1.0]), name='sexp') for _ in range(d)],
                         [kernel(length=np.array([1.0]), name='matern2.5', scale_est=True, connect=np.arange(d))])
        m = dgp(X, Y, layers, vecchia=True, m=10, seed=8)
        used = []
        inner = m._mstep_can_start_early
        m._mstep_can_start_early = lambda: used.append(inner()) or used[-1]
        m.train(N=5, ess_burn=3, disable=True)
        return m, used

    a, ua = run('1', '2')
    b, ub = run('0', '1')
    assert ua == [True] * 5 and ub == [False] * 5   # (the refresh iterations 2 and 4 as well: their diagnostics run behind the first launches)
    for la, lb in zip(a.all_layer, b.all_layer):
        for na, nb in zip(la, lb):
            assert np.array_equal(na.para_path, nb.para_path)
            assert np.array_equal(na.length, nb.length) and np.array_equal(na.scale, nb.scale) and np.array_equal(na.nugget, nb.nugget)
            assert np.array_equal(na.output, nb.output) and np.array_equal(na.input, nb.input)
            assert np.array_equal(na.ord, nb.ord) and np.array_equal(na.NNarray, nb.NNarray) and np.array_equal(na.rev_ord, np.argsort(na.ord))
            if getattr(na, 'R2', None) is not None:
                assert np.array_equal(np.asarray(na.R2), np.asarray(nb.R2))


def test_dense_training_does_not_depend_on_the_early_mstep_start(eng, monkeypatch):
    """dgp.train on a dense model (round 6) queues the M-step's first round of objective evaluations from the imputer's device state
    (dgpamd_llik_batch_launch) and refreshes the nodes' numpy attributes / runs the R2 diagnostics while the device works on it
    (imputer.sample(detach=False), dgp._mstep_can_start_early, mstep.maximise_lockstep(after_first_launch=...)).  A schedule, not an
    algorithm: hyper-parameters, paths, latents, node inputs and R2 after six iterations equal the plain order's, bit for bit --
    dgp.py:1377-1398 in the reference's order.  Models the early start must refuse (a reference prior upstairs) take the plain order."""
    from dgp_amd import dgp, kernel, combine
    rng = np.random.default_rng(21)
    n, d = 300, 3
    X = rng.uniform(size=(n, d))
    f = np.sin(4 * X[:, 0]) * np.cos(3 * X[:, 1]) + 0.5 * X[:, 2] ** 2
    Y = ((f - f.mean()) / f.std())[:, None]

    def run(early, prior='ga'):
        monkeypatch.setenv('DGPAMD_MSTEP_EARLY', early)
        np.random.seed(3)
        layers = combine([kernel(length=np.array([1.0]), name='matern2.5') for _ in range(d)],
                         [kernel(length=np.array([1.0]), name='matern2.5', scale_est=True, connect=np.arange(d), prior_name=prior)])
        m = dgp(X, Y, layers, seed=8)
        used = []
        inner = m._mstep_can_start_early
        m._mstep_can_start_early = lambda: used.append(inner()) or used[-1]
        m.train(N=6, ess_burn=4, disable=True)
        return m, used

    a, ua = run('1')
    b, ub = run('0')
    assert ua == [True] * 6 and ub == [False] * 6
    for la, lb in zip(a.all_layer, b.all_layer):
        for na, nb in zip(la, lb):
            assert np.array_equal(na.para_path, nb.para_path)
            assert np.array_equal(na.length, nb.length) and np.array_equal(na.scale, nb.scale) and np.array_equal(na.nugget, nb.nugget)
            assert np.array_equal(na.output, nb.output) and np.array_equal(na.input, nb.input)
            if getattr(na, 'R2', None) is not None:
                assert np.array_equal(np.asarray(na.R2), np.asarray(nb.R2))
    c, uc = run('1', prior='ref')
    assert uc == [False] * 6


def test_one_si_iteration_at_bench_size_vs_oracle(eng):
    """ONE stochastic-imputation iteration of BASELINE's configs[1] (n = 2000, d = 5, 5 + 1 Matern-2.5 nodes) against
    the oracle with injected draws: the I-step's block update (prior draws through five n x n factors, the speculative
    batch's twelve factorisations, the device-resident accept / shrink loop) must accept the proposal the sequential
    sampler accepts and consume the same uniforms; the M-step's objective and gradient (K assembly, factorisation + fused
    inverse, derivative reductions) must agree at the resulting state.  Oracle: ~0.5 s per n = 2000 log-likelihood."""
    from oracle import dgp_oracle as O
    from dgp_amd.imputation import DrawStream
    import bench
    model, X, Y = bench.build_model(2000, 5, 100, 0)
    model.engine = eng
    n, d = X.shape
    rng = np.random.default_rng(77)
    z = [rng.standard_normal(n) for _ in range(d)]
    u = list(rng.random(40))
    imp = model.imp
    imp.draws = DrawStream(z=[v.copy() for v in z], u=list(u))
    layer0, top = model.all_layer[0], model.all_layer[1][0]
    F0 = np.stack([nd.output[:, 0] for nd in layer0], 1)
    par = dict(length=top.length.copy(), scale=float(top.scale[0]), nugget=float(top.nugget[0]))
    nu = np.stack([O.fmvn(float(nd.scale[0]) * O.k_matrix(nd.input, nd.length, nd.nugget[0], nd.name), z[k]) for k, nd in enumerate(layer0)], 1)

    def upper(fp):
        Xi = np.concatenate((fp[:, top.input_dim], X[:, top.connect]), 1)
        return O.log_likelihood(Xi, Y, par['length'], par['scale'], par['nugget'], top.name)

    f_ref, nprop, thetas, lls, log_y = O.ess_block_sweep(F0, nu, upper, np.log(u[0]), u[1:])
    imp.sample(burnin=0)
    F1 = np.stack([nd.output[:, 0] for nd in layer0], 1)
    assert len(imp.draws._ubuf) == len(u) - (1 + nprop), 'uniforms consumed: threshold + one per proposal'
    close(F1, f_ref, rtol=1e-8, atol=1e-10)
    # the accepted state's log-likelihood as the device computed it (the threshold of the next update)
    close(imp._ll_cache[0], lls[-1], rtol=1e-9)
    # M-step objective / gradient of every node at this state
    for l, layer in enumerate(model.all_layer):
        for nd in layer:
            nd.engine = eng
            if l != 0:
                nd.r2()
            x = nd.log_t()
            Xn = nd.input if nd.global_input is None else np.concatenate((nd.input, nd.global_input), 1)
            nll_o, g_o, _ = O.nll_grad(x, Xn, nd.output, nd.name, nd.scale.copy(), nd.nugget[0], nd.nugget_est, nd.scale_est,
                                       nd.prior_name, nd.prior_coef, getattr(nd, 'cl', None), None, None, None)
            sc = nd.scale.copy()
            nll, g = nd.llik(x.copy())
            nd.scale = sc
            # Bounds set by the measured evaluation-to-evaluation noise of BOTH objectives at this size and conditioning
            # (profiles/r04_mstep_tail.txt: 1e-7 .. 6e-7 absolute on |nll| ~ 8e3 for the oracle, 0.4e-7 .. 2e-7 for the device;
            # their difference stays below 5e-7): 4e-6 absolute here (rtol 5e-10), eight times the largest difference seen;
            # gradient entries within 2e-5 + 1e-7 |g| of the oracle's (its own spread reaches 7e-6).
            close(nll, nll_o, rtol=5e-10)
            close(g, g_o, rtol=1e-7, atol=2e-5)


def test_device_objective_noise_is_not_larger_than_the_oracles(eng):
    """L-BFGS-B's line searches near a fit's optimum are decided by differences of the objective that are
    as small as its evaluation-to-evaluation noise (kernel_class.py:537-545: maxfun = max(30, 20 + 5 D) is reached by a node
    whose line search keeps failing), so the device's noise must not exceed the reference formulation's -- otherwise its
    M-step tail would be longer than LAPACK's.  n = 2000, d = 5, Matern-2.5, nugget 1e-6 (cond ~ 1e7): 20 evaluations of
    kernel.llik at x (1 + j 1e-13), j = -10 .. 9, against the oracle's at eight of those points -- the spread of the value and
    of every gradient entry at most 3 times the oracle's (measured: 0.4 .. 1 times, profiles/r04_mstep_tail.txt)."""
    from oracle import dgp_oracle as O
    import bench
    model, X, Y = bench.build_model(2000, 5, 100, 0)
    model.engine = eng
    model.imp.sample(burnin=2)
    for nd in (model.all_layer[0][1], model.all_layer[1][0]):
        nd.engine = eng
        if nd is model.all_layer[1][0]:
            nd.r2()
        x = nd.log_t()
        Xn = nd.input if nd.global_input is None else np.concatenate((nd.input, nd.global_input), 1)
        sc = nd.scale.copy()
        fd, gd, fo, go = [], [], [], []
        for j in range(-10, 10):
            xj = x * (1.0 + j * 1e-13)
            f, g = nd.llik(xj.copy())
            nd.scale = sc.copy()
            fd.append(float(np.ravel(f)[0])); gd.append(np.array(g, float))
            if j % 3 == 0 or j == 9:   # eight of the twenty points: ~0.4 s each
                f0, g0, _ = O.nll_grad(xj, Xn, nd.output, nd.name, sc.copy(), nd.nugget[0], nd.nugget_est, nd.scale_est,
                                       nd.prior_name, nd.prior_coef, getattr(nd, 'cl', None), None, None, None)
                fo.append(float(np.ravel(f0)[0])); go.append(np.array(g0, float))
        sf_d, sf_o = np.ptp(fd), np.ptp(fo)
        sg_d, sg_o = np.ptp(np.stack(gd), axis=0), np.ptp(np.stack(go), axis=0)
        # (floors: eight oracle points can fall close together by chance; 1e-7 / 1e-6 are its typical spreads)
        assert sf_d <= 3.0 * max(sf_o, 1e-7), (sf_d, sf_o)
        assert np.all(sg_d <= 3.0 * np.maximum(sg_o, 1e-6)), (sg_d, sg_o)
        assert abs(np.mean(fd) - np.mean(fo)) <= 5e-10 * abs(np.mean(fo))


def test_node_inputs_written_in_place_are_honoured(eng):
    """The reference's own sampler writes node.input[:, idx] in place (imputation.py:160-202), and so may code written against
    it.  Rounds 2-3 froze those arrays (flags.writeable = False -> ValueError); now they are plain writable arrays and an
    array that has been handed out is compared by value: an in-place edit of a first-layer input between two iterations must
    reach the device copy, drop the cached prior factors and change what the sampler draws; an in-place edit of an upper
    node's input after an I-step must reach that node's M-step objective."""
    from dgp_amd import dgp, kernel, combine
    rng = np.random.default_rng(4)
    n, d = 120, 2
    X = rng.uniform(size=(n, d))
    Y = np.sin(4 * X[:, [0]]) + X[:, [1]] ** 2
    layers = combine([kernel(length=np.array([1.0]), name='matern2.5') for _ in range(d)],
                     [kernel(length=np.array([1.0]), name='matern2.5', scale_est=True, connect=np.arange(d))])
    model = dgp(X, Y, layers, seed=5)
    imp = model.imp
    nd0, top = model.all_layer[0][0], model.all_layer[1][0]
    assert nd0._private('input')                      # the model's own copy: recognised by identity
    imp.sample(burnin=1)
    assert nd0._private('input') and imp._const_same(('x', 0), nd0._input, True)
    a = nd0.input                                     # handed out ...
    assert a.flags.writeable and not nd0._private('input')
    a[:, 0] += 0.25                                   # ... and written in place
    assert not imp._const_same(('x', 0), nd0._input, nd0._private('input'))
    imp.sample(burnin=1)
    np.testing.assert_array_equal(imp._x0[0].cpu().numpy(), a)      # the device copy follows
    assert imp._const_same(('x', 0), nd0._input, nd0._private('input'))
    # upper node: _detach has just bound a private copy of the latents as its input
    assert top._private('input')
    pre = imp.stage_for_mstep()
    assert id(top) in pre                             # device views are handed to the M-step while nothing was touched
    x = top.log_t()
    top.engine = eng
    f0, _ = top.llik(x.copy())
    top.input[:, 0] = top.input[::-1, 0].copy()       # the reference's idiom: node.input[:, idx] = ...
    assert id(top) not in imp.stage_for_mstep()       # the edit is seen: this node stages from its numpy arrays again
    top._staged = None
    f1, _ = top.llik(x.copy())
    assert abs(float(np.ravel(f1)[0]) - float(np.ravel(f0)[0])) > 1e-6


def test_rccl_first_contact_world_one(tmp_path):
    """The `nccl` backend (RCCL) on the one-GPU box: a process group of ONE rank that the library is told to treat as active
    (DGPAMD_DIST_FORCE=1), so that every collective helper of dgp_amd/dist.py, the sharded emulator.predict (imputations:
    one all-reduce, emulation.py:846-847; points: one all-gather, emulation.py:603-613), the node-split M-step (one
    all-gather of doubles, dgp.py:1455-1467) and the row-split Vecchia evaluations (one all-reduce per evaluation / batch,
    vecchia.py:165-242) really go through RCCL on device tensors -- everything else that is known about these paths comes
    from gloo.  With one rank every collective is an identity, so the results must equal the unsharded ones exactly."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / 'worker.py'
    script.write_text("""
import os, sys, faulthandler
faulthandler.dump_traceback_later(200, exit=True)
sys.path.insert(0, %r)
import numpy as np, torch, copy
from dgp_amd import dgp, kernel, combine, emulator, dist as dd
dd.init_from_env('nccl')
import torch.distributed as td
assert td.is_initialized() and td.get_backend() == 'nccl' and td.get_world_size() == 1 and dd.is_active()
dev = torch.device('cuda', 0)
# ---- every helper, on device tensors where RCCL wants them
dd.barrier()
a, b = torch.arange(6, dtype=torch.float64, device=dev), torch.ones(3, 2, dtype=torch.float64, device=dev)
dd.allreduce_sum(a, b)
assert a.tolist() == [0, 1, 2, 3, 4, 5] and float(b.sum()) == 6.0
h = torch.ones(4, dtype=torch.float64)           # a host tensor under nccl: round trip through the device
dd.allreduce_sum(h)
assert h.tolist() == [1, 1, 1, 1]
assert dd.allreduce_max_scalar(2.5) == 2.5 and dd.allreduce_max_scalar(-1.0, dev) == -1.0
rows = np.arange(21.0).reshape(7, 3)
assert np.array_equal(dd.allgather_rows(rows, 7), rows) and np.array_equal(dd.allgather_rows(rows, 7, dev), rows)
assert np.array_equal(dd.allgather_vector(np.array([1.0, 2.0, 3.0])), [[1.0, 2.0, 3.0]])
assert dd.allreduce_sum_vector(torch.full((5,), 2.0, dtype=torch.float64, device=dev)).tolist() == [2.0] * 5
big = (1 << 127) + 12345678901234567890
assert dd.broadcast_int(big) == big and dd.broadcast_int(7, device=dev) == 7
assert dd.allgather_objects({'r': dd.rank()}) == [{'r': 0}]
print('helpers ok', flush=True)
# ---- prediction: imputations sharded / points sharded == unsharded
rng = np.random.default_rng(3)
X = rng.uniform(size=(150, 3)); Y = np.sin(4 * X[:, [0]]) + X[:, [1]] * X[:, [2]]
def layers():
    return combine([kernel(length=np.array([1.0]), name='matern2.5') for _ in range(3)],
                   [kernel(length=np.array([1.0]), name='matern2.5', scale_est=True, connect=np.arange(3))])
m = dgp(X, Y, layers(), seed=7)
m.train(N=3, ess_burn=2, disable=True)
est = m.estimate()
xt = rng.uniform(size=(37, 3))
ref = emulator(copy.deepcopy(est), N=4, seed=9, shard=False).predict(xt)
sh = emulator(copy.deepcopy(est), N=4, seed=9)
assert sh.shard and sh.N == 4
mu, var = sh.predict(xt)
assert np.array_equal(mu, ref[0]) and np.array_equal(var, ref[1])
pt = emulator(copy.deepcopy(est), N=4, seed=9, shard='points')
assert pt.shard_points
mu, var = pt.predict(xt)
assert np.array_equal(mu, ref[0]) and np.array_equal(var, ref[1])
assert emulator(copy.deepcopy(est), N=2, shard='points').N == 2     # (seed broadcast as device words)
print('prediction ok', flush=True)
# ---- node-split M-step == unsplit
def hyper(model):
    return np.concatenate([np.concatenate((nd.scale, nd.length, nd.nugget)) for layer in model.all_layer for nd in layer])
def dense(split):
    dd.split_training(rows=False, nodes=split)
    mm = dgp(X, Y, layers(), seed=7)
    mm.train(N=3, ess_burn=2, disable=True)
    return mm
assert np.array_equal(hyper(dense(True)), hyper(dense(False)))
dd.split_training(nodes=False)
print('node split ok', flush=True)
# ---- Vecchia rows split: evaluations, one M-step, one I-step
Xv = rng.uniform(size=(260, 2)); Yv = np.sin(5 * Xv[:, [0]]) + Xv[:, [1]] ** 2
def vecch():
    np.random.seed(5)
    ls = combine([kernel(length=np.array([1.0]), name='sexp') for _ in range(2)],
                 [kernel(length=np.array([1.0]), name='sexp', scale_est=True, connect=np.arange(2))])
    return dgp(Xv, Yv, ls, seed=9, vecchia=True, m=8)
c, d = vecch(), vecch()
dd.split_training(rows=True)
q0 = c.imp.queued_calls
np.random.seed(11); c.imp.sample(burnin=2)
assert c.imp.queued_calls == q0 + 1        # the device queue runs under the split: RCCL sums every batch's partial sums on the stream
c._m_step()
dd.split_training(rows=False)
np.random.seed(11); d.imp.sample(burnin=2); d._m_step()
# (one rank: its block of rows is all rows and the all-reduce an identity -- the same launches, the same bits)
for lc, ld_ in zip(c.all_layer, d.all_layer):
    for nc, nd_ in zip(lc, ld_):
        assert np.array_equal(nc.output, nd_.output)
assert np.array_equal(hyper(c), hyper(d))
print('rows split ok', flush=True)
dd.barrier()
td.destroy_process_group()
print('rank 0 ok')
""" % root)
    env = dict(os.environ, DGPAMD_DIST_FORCE='1', MASTER_ADDR='127.0.0.1', MASTER_PORT='29553', WORLD_SIZE='1', RANK='0',
               LOCAL_RANK='0', HSA_ENABLE_IPC_MODE_LEGACY='0')
    p = subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    try:
        out = p.communicate(timeout=400)[0].decode()
    except subprocess.TimeoutExpired:
        p.kill()
        raise AssertionError('RCCL worker timed out:\n' + p.communicate()[0].decode()[-3000:])
    assert p.returncode == 0, out[-4000:]
    assert 'rank 0 ok' in out


def test_training_splits_two_ranks(tmp_path):
    """The two natural multi-GPU splits of TRAINING one model (dist.split_training) on two processes (gloo
    rendezvous, both on this GPU, same seed = same draws): Vecchia likelihood rows n/2 per rank with an all-reduce of
    (quad, logdet, gradient) (vecchia.py:164-242), and M-step nodes round-robin with one all-gather of the fitted
    hyper-parameters (dgp.py:1455-1467).  Both must reproduce the single-rank training: rows to 1e-10 (a different
    summation order), nodes bit for bit.  The I-step runs with the rows split as well (one all-reduce per speculative batch):
    both ranks must end with the same latents."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / 'worker.py'
    script.write_text("""
import os, sys, faulthandler
faulthandler.dump_traceback_later(100, exit=True)   # (a stuck rank says where)
sys.path.insert(0, %r)
import numpy as np
from dgp_amd import dgp, kernel, combine, dist as dd
dd.init_from_env('gloo')
rng = np.random.default_rng(3)

def hyper(model):
    return np.concatenate([np.concatenate((nd.scale, nd.length, nd.nugget)) for layer in model.all_layer for nd in layer])

# ---- dense model: M-step nodes split
X = rng.uniform(size=(150, 3)); Y = np.sin(4 * X[:, [0]]) + X[:, [1]] * X[:, [2]]
def dense(split):
    dd.split_training(rows=False, nodes=split)
    layers = combine([kernel(length=np.array([1.0]), name='matern2.5') for _ in range(3)],
                     [kernel(length=np.array([1.0]), name='matern2.5', scale_est=True, connect=np.arange(3))])
    m = dgp(X, Y, layers, seed=7)
    m.train(N=3, ess_burn=2, disable=True)
    return m
a = dense(True); print('nodes split trained', flush=True)
b = dense(False); print('unsplit trained', flush=True)
assert np.array_equal(hyper(a), hyper(b)), (hyper(a), hyper(b))
for la, lb in zip(a.all_layer, b.all_layer):
    for na, nb in zip(la, lb):
        assert np.array_equal(na.para_path, nb.para_path)

# ---- Vecchia model: likelihood rows split.  Every objective / gradient / log-likelihood evaluation must agree with the
# unsplit one to rounding (a different summation order); one M-step from the same state ends within the optimiser's own
# tolerance (L-BFGS-B stops on a flat objective: 1e-16 in f moves its last iterate by ~1e-6).  Whole trainings are not
# compared: the SI chain amplifies such differences (a flipped accept decision) like any change of rounding would.
Xv = rng.uniform(size=(260, 2)); Yv = np.sin(5 * Xv[:, [0]]) + Xv[:, [1]] ** 2
def vecch():
    np.random.seed(5)   # the Vecchia ordering is drawn from numpy's global generator (as in the reference): same on every rank / run
    layers = combine([kernel(length=np.array([1.0]), name='sexp') for _ in range(2)],
                     [kernel(length=np.array([1.0]), name='sexp', scale_est=True, connect=np.arange(2))])
    return dgp(Xv, Yv, layers, seed=9, vecchia=True, m=8)
dd.split_training(rows=False, nodes=False)
c, d = vecch(), vecch()
for l, layer in enumerate(c.all_layer):
    for nd in layer:
        nd.engine = c.engine
        if l != 0:
            nd.r2()
        x, sc = nd.log_t(), nd.scale.copy()
        dd.split_training(rows=False)
        f0, g0 = nd.llik_vecch(x.copy()); s0 = nd.scale.copy(); nd.scale = sc.copy()
        l0 = nd.log_likelihood_func_vecch()
        dd.split_training(rows=True)
        f1, g1 = nd.llik_vecch(x.copy()); s1 = nd.scale.copy(); nd.scale = sc.copy()
        l1 = nd.log_likelihood_func_vecch()
        np.testing.assert_allclose(f1, f0, rtol=1e-12); np.testing.assert_allclose(g1, g0, rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(s1, s0, rtol=1e-12); np.testing.assert_allclose(l1, l0, rtol=1e-12)
print('evaluations agree', flush=True)
dd.split_training(rows=True)
np.random.seed(11); c._m_step()
print('rows split m-step done', flush=True)
dd.split_training(rows=False)
np.random.seed(11); d._m_step()
np.testing.assert_allclose(hyper(c), hyper(d), rtol=1e-4, atol=1e-8)
# the I-step with the rows split: every speculative batch's sums are all-reduced, so both ranks must take the same accept
# decisions and end with the same latent layer, bit for bit
dd.split_training(rows=True)
q0 = c.imp.queued_calls
c.imp.sample(burnin=2)
assert c.imp.queued_calls == q0 + 1, 'the device queue was not used under the rows split'   # (the reduce hook sums the batches' partial sums)
Fc = np.concatenate([nd.output for nd in c.all_layer[0]], 1)
assert np.all(np.isfinite(Fc))
both = dd.allgather_objects(Fc.tobytes())
assert both[0] == both[1], 'the ranks ended with different latents'
dd.split_training(rows=False)
# the same I-step on all rows (same draws): the same accept decisions unless a threshold falls inside the rounding of a sum
e_ = vecch(); e_.imp.draws = type(e_.imp.draws)(seed=123); f_ = vecch(); f_.imp.draws = type(f_.imp.draws)(seed=123)
dd.split_training(rows=True); e_.imp.sample(burnin=3); dd.split_training(rows=False); f_.imp.sample(burnin=3)
np.testing.assert_allclose(np.concatenate([nd.output for nd in e_.all_layer[0]], 1), np.concatenate([nd.output for nd in f_.all_layer[0]], 1), rtol=0, atol=1e-9)
assert e_.imp.stats['proposals'] == f_.imp.stats['proposals']
print('rows split i-step agrees across ranks', flush=True)
dd.barrier()
print('rank', dd.rank(), 'ok')
""" % root)
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT='29549', WORLD_SIZE='2')
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r), LOCAL_RANK='0'),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(2)]
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=120)[0].decode())
    except subprocess.TimeoutExpired:   # (a rank that died leaves the other waiting in a collective: end both, show what they said)
        for p in procs:
            p.kill()
        outs = [p.communicate()[0].decode()[-3000:] for p in procs]
        raise AssertionError('two-rank worker timed out:\n' + '\n----\n'.join(outs))
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o
        assert 'ok' in o
