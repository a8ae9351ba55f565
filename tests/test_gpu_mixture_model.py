"""predict_dist / loo_dist of emulator, gp and lgp: the predictive mixture built from the models' own per-imputation moments.
Small models (n <= 60, N <= 4).  Needs an MI355X: -m gpu."""
import functools
import warnings

import numpy as np
import pytest
from scipy.special import ndtri

import mixture_ref as R
from test_gpu_pathfun import _gp, _model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    from dgp_amd.ops import Engine
    return Engine(0)


@functools.lru_cache(maxsize=None)
def trained(which):
    return _model(which)


def emu_of(which, N=4):
    from dgp_amd import emulator
    X, model = trained(which)
    return X, emulator(model.estimate(), N=N, seed=1)


def columns(mu_s, v_s):
    """predict(aggregation=False)'s lists as (S, M*K) arrays."""
    return np.stack(mu_s).reshape(len(mu_s), -1), np.stack(v_s).reshape(len(v_s), -1)


def within(out, ref, bound, what):
    ratio = float((np.abs(out - ref) / bound).max())
    print('%s: max difference / bound = %.3g' % (what, ratio))
    assert ratio <= 1.0, (what, ratio)


@pytest.mark.parametrize('vecchia', [False, True])
def test_emulator_predict_dist(eng, vecchia):
    X, emu = emu_of('two-connect')
    if vecchia:
        emu.to_vecchia()
    rng = np.random.default_rng(3)
    x = rng.uniform(size=(70, 2))
    dist = emu.predict_dist(x, m=25)
    mu, var = emu.predict(x, m=25)
    assert (dist.S, dist.M, dist.K) == (4, 70, 1)
    assert np.array_equal(dist.mean(), mu) and np.array_equal(dist.var(), var)
    ms, vs = columns(*emu.predict(x, m=25, aggregation=False))
    # the numpy formulas on the per-imputation lists are themselves rounded: two bounds (C = 8 each, device and numpy)
    y = mu + np.sqrt(var) * rng.normal(size=mu.shape)
    b_cdf = np.array([R.cdf_bound(ms[:, i], vs[:, i], y.reshape(-1)[i]) for i in range(70)]).reshape(70, 1)
    cdf = dist.cdf(y)
    within(cdf, R.np_cdf(ms, vs, y.reshape(-1)).reshape(70, 1), 2 * b_cdf, 'cdf vs numpy')
    within(dist.sf(y), 1.0 - cdf, 2 * b_cdf + 2.0 ** -52, 'sf vs 1 - cdf')
    assert dist.cdf(np.array([-1e3, 1e3])).shape == (70, 1, 2) and dist.logpdf(y[:, :, None]).shape == (70, 1, 1)
    b_crps = np.array([R.crps_bound(ms[:, i], vs[:, i], y.reshape(-1)[i]) for i in range(70)]).reshape(70, 1)
    within(dist.crps(y), R.np_crps(ms, vs, y.reshape(-1)).reshape(70, 1), 2 * b_crps, 'crps vs numpy')
    p = np.array([0.025, 0.2, 0.5, 0.9, 0.975])
    q = dist.quantile(p)
    assert q.shape == (70, 1, 5) and dist.quantile(0.5).shape == (70, 1)
    assert np.array_equal(dist.quantile(0.5), q[:, :, 2])
    for i in range(0, 70, 7):   # the quantile statement against the exact cdf of the numpy lists
        for t, pp in enumerate(p):
            ok, _, text = R.quantile_check(ms[:, i], vs[:, i], pp, q[i, 0, t])
            assert ok, (i, pp, text)
    back = dist.cdf(q)          # cdf(quantile(p)) returns p within the cdf bound (at q, plus delta's worth of density)
    for i in range(70):
        for t, pp in enumerate(p):
            slack = R.cdf_bound(ms[:, i], vs[:, i], q[i, 0, t]) + float(R.pdf(ms[:, i], vs[:, i], q[i, 0, t])) * R.quantile_delta(ms[:, i], q[i, 0, t])
            assert abs(back[i, 0, t] - pp) <= 2 * slack, (i, pp, back[i, 0, t], slack)
    lo, hi = dist.interval(0.95)
    ends = dist.quantile(np.array([0.5 * (1 - 0.95), 0.5 * (1 + 0.95)]))    # one quantile call with two probabilities
    assert np.array_equal(lo, ends[:, :, 0]) and np.array_equal(hi, ends[:, :, 1])
    assert np.all(lo <= q[:, :, 2]) and np.all(q[:, :, 2] <= hi)


@pytest.mark.parametrize('vecchia', [False, True])
def test_loo_dist_has_loo_s_moments(eng, vecchia):
    X, emu = emu_of('two-connect', N=3)
    if vecchia:
        emu.to_vecchia()
    mu, var = emu.loo(X, m=20)
    dist = emu.loo_dist(X, m=20)
    assert (dist.S, dist.M, dist.K) == (3, len(X), 1)
    assert np.array_equal(dist.mean(), mu) and np.array_equal(dist.var(), var)
    _, model = trained('two-connect')
    pit = dist.cdf(model.Y)
    assert pit.shape == mu.shape and np.all((pit >= 0) & (pit <= 1))
    lo, hi = dist.interval(0.9)
    assert np.all(lo < hi) and np.all(dist.crps(model.Y) >= 0)


def test_gp_predict_dist_is_the_one_gaussian(eng):
    rng = np.random.default_rng(8)
    X = rng.uniform(size=(60, 3))
    Y = (np.sin(3 * X[:, 0]) + X[:, 1] * X[:, 2] + 0.05 * rng.normal(size=60))[:, None]
    m = _gp('matern2.5', X, Y)
    x = rng.uniform(size=(65, 3))
    dist = m.predict_dist(x)
    mu, s2 = m.predict(x)
    assert (dist.S, dist.M, dist.K) == (1, 65, 1)
    assert np.array_equal(dist.mean(), mu)
    p = np.array([1e-12, 0.025, 0.5, 0.975, 1 - 1e-12])
    q = dist.quantile(p)[:, 0, :]
    zs = ndtri(p)[None, :] * np.sqrt(s2)
    ulp = np.spacing(np.maximum(np.abs(mu), np.abs(zs)))   # (the rounding of the sum's larger operand)
    assert np.all(np.abs(q - (mu + zs)) <= 4 * ulp)
    y = mu + 0.7 * np.sqrt(s2)
    b = np.array([R.cdf_bound(mu[i], s2[i], y[i, 0]) for i in range(65)])[:, None]
    within(dist.cdf(y), R.np_cdf(mu[None], s2[None], y), 2 * b, 'gp cdf')


# lgp.predict of the golden GP -> DGP -> GP chain (tests/golden/g10_lgp_sexp.npz) at its first three test points, as the build whose
# expanded SExp pair forms take their coordinates relative to W[0] (csrc/linkgp.hpp, CENTRE) returns it on an MI355X.  The pin guards
# predict's walk, shared with predict_dist, against changes of a bit; it was recorded first on the commit before the walk was shared, as
#   ['0x1.929faf534ee90p-1', '0x1.ace5fc2199300p+0', '0x1.92829906cb510p+0'], ['0x1.7b9ee6581cf80p-7', '0x1.04cba33a5bf40p-5', '0x1.fa9f2b3e14100p-5']
# and recorded again when the centring changed the last bits of the SExp J sums: these variances by up to 2.5e-9 (2.2e-7 relative; the
# chain's nuggets are 1e-6, cond(R) ~ 1e6), these means, which the inner layers' variances feed, by up to 3.3e-10.  The golden chain itself
# is held to 1e-6 / 1e-8 and 1e-5 / 1e-6 (tests/test_gpu_model.py, test_linked_chain_matches_reference).
LGP_PARENT = (['0x1.929faf5618c2fp-1', '0x1.ace5fc2186e25p+0', '0x1.92829906c68b8p+0'],
              ['0x1.7b9eebb4a1a00p-7', '0x1.04cba33b8d800p-5', '0x1.fa9f2b3632340p-5'])


def test_lgp_predict_dist(eng, golden):
    from test_gpu_lgp_paths import _chain
    sysm, xin = _chain(eng, golden, 'sexp')
    mu, var = sysm.predict(xin)
    dists = sysm.predict_dist(xin)
    assert len(dists) == len(mu) == 1
    d = dists[0]
    assert (d.S, d.M, d.K) == (len(sysm.all_layer_set), len(xin[0]), 1)
    assert np.array_equal(d.mean(), mu[0]) and np.array_equal(d.var(), var[0])
    print('lgp.predict: mean %s var %s' % ([float(v).hex() for v in mu[0][:3, 0]], [float(v).hex() for v in var[0][:3, 0]]))
    assert [float(v).hex() for v in mu[0][:3, 0]] == LGP_PARENT[0] and [float(v).hex() for v in var[0][:3, 0]] == LGP_PARENT[1]
    lo, hi = d.interval(0.95)
    med = d.quantile(0.5)
    assert np.all(lo <= med) and np.all(med <= hi)
    cdf = d.cdf(med)
    assert np.all(np.abs(cdf - 0.5) < 1e-12)


def test_refusals(eng):
    from dgp_amd import container, lgp
    X, emu = emu_of('two-connect', N=2)
    with pytest.raises(Exception, match='The testing input has to be a numpy 2d-array'):
        emu.predict_dist(X[:, 0])
    dist = emu.predict_dist(X[:5])
    for bad in (0.0, 1.0, -0.2, np.array([0.5, 1.5]), np.nan):
        with pytest.raises(ValueError):
            dist.quantile(bad)
    with pytest.raises(ValueError):
        dist.interval(1.0)
    with pytest.raises(Exception, match='y has to be a numpy array of shape'):
        dist.cdf(np.zeros((4, 1)))
    with pytest.raises(Exception, match='y has to be a numpy array of shape'):
        dist.crps(np.zeros(5))
    emu.shard = True
    try:
        with pytest.raises(NotImplementedError, match='sharded over ranks'):
            emu.predict_dist(X[:5])
        with pytest.raises(NotImplementedError, match='sharded over ranks'):
            emu.loo_dist(X)
    finally:
        emu.shard = False
    for which in ('hetero', 'categorical'):
        Xl, lik = emu_of(which, N=2)
        with pytest.raises(ValueError, match="predict\\(method='sampling'\\)"):
            lik.predict_dist(Xl[:5])
        with pytest.raises(ValueError, match="predict\\(method='sampling'\\)"):
            lik.loo_dist(Xl)
    _, het = trained('hetero')
    rng = np.random.default_rng(2)
    X1 = rng.uniform(size=(30, 1))
    first = _gp('sexp', X1, np.sin(4 * X1))
    sysm = lgp([[container(first.export(), local_input_idx=np.array([0]))],
                [container(het.estimate(), local_input_idx=np.array([0]))]], N=2)
    with pytest.raises(ValueError, match="predict\\(method='sampling'\\)"):
        sysm.predict_dist(X1[:4])
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        from dgp_amd.mixture import PredictiveMixture
        with pytest.raises(ValueError, match='NaN'):
            PredictiveMixture(eng, eng.tensor(np.full((2, 3, 1), np.nan)), eng.tensor(np.ones((2, 3, 1))))
