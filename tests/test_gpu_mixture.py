"""The predictive-mixture kernels (csrc/mixture.hip through Engine.mixture_eval / _quantile / _crps) against the mpmath reference
of tests/mixture_ref.py, within the bounds stated there (C = 8), and bit for bit across slices and kernel forms.

The device runs every entry of a case; the exact reference, which is slow, is taken at a fixed choice of entries: the first and
last, the neighbours of the 64-entry workgroup edges, and a few more by a seeded draw.  Every test prints its largest
error / bound before it asserts.  Needs an MI355X: -m gpu."""
import numpy as np
import pytest
from scipy.special import ndtri

import mixture_ref as R

pytestmark = pytest.mark.gpu

P5 = np.array([1e-12, 0.025, 0.5, 0.975, 1 - 1e-12])


@pytest.fixture(scope='module')
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    from dgp_amd.ops import Engine
    return Engine(0)


def npy(t):
    return t.detach().cpu().numpy()


def chosen(count, k, seed=0):
    """At most ~k + 8 entries of range(count): the ends, the workgroup edges, k by a seeded draw."""
    fixed = [i for i in (0, 1, 62, 63, 64, 65, 127, 128, count - 1) if 0 <= i < count]
    rng = np.random.default_rng(seed)
    return sorted(set(fixed) | set(rng.integers(0, count, size=min(k, count)).tolist()))


def few(count):
    """The entries of a case with many components that are checked exactly: the first, the last of the first workgroup, the last."""
    return sorted({0, min(63, count - 1), count - 1})


def mixtures(S, count, seed, spread=3.0):
    rng = np.random.default_rng(seed)
    mu = spread * rng.normal(size=(S, count))
    var = np.exp(rng.normal(size=(S, count)))
    return mu, var


def thresholds(mu, var, T, seed):
    """Per entry T thresholds: draws from the mixture itself and points out in its tails."""
    rng = np.random.default_rng(seed)
    S, count = mu.shape
    s = rng.integers(0, S, size=(count, T))
    e = np.arange(count)[:, None]
    return mu[s, e] + np.sqrt(np.maximum(var[s, e], 0)) * rng.normal(size=(count, T)) * rng.choice([0.3, 1.0, 4.0], size=(count, T))


def check_eval(eng, what, mu, var, y, entries, label):
    """Engine.mixture_eval(what) on all entries against the reference at `entries`.  y: (count, T) or (T,)."""
    out = npy(eng.mixture_eval(what, eng.tensor(mu), eng.tensor(var), eng.tensor(y)))
    assert out.shape == (mu.shape[1], y.shape[-1])
    ref = dict(cdf=R.cdf, sf=R.sf, logpdf=R.logpdf)[what]
    bound = dict(cdf=R.cdf_bound, sf=lambda *a: R.cdf_bound(*a, upper=True), logpdf=R.logpdf_bound)[what]
    worst, where = 0.0, None
    for e in entries:
        for t in range(y.shape[-1]):
            yy = y[e, t] if y.ndim == 2 else y[t]
            exact = ref(mu[:, e], var[:, e], yy)
            if exact == R.mp.mpf('-inf'):
                assert out[e, t] == -np.inf, (label, e, t, out[e, t])
                continue
            ratio = float(abs(R.mp.mpf(float(out[e, t])) - exact)) / bound(mu[:, e], var[:, e], yy)
            if ratio > worst:
                worst, where = ratio, (e, t, out[e, t], float(exact))
    print('%s %s: max error / bound = %.3g at %s' % (label, what, worst, where))
    assert worst <= 1.0, (label, what, worst, where)
    return out


def check_quantile(eng, mu, var, p, entries, label, path=None):
    out, capped = eng.mixture_quantile(eng.tensor(mu), eng.tensor(var), p, path=path)
    out = npy(out)
    assert out.shape == (mu.shape[1], len(p))
    assert capped == 0, (label, capped)
    worst = 0.0
    for e in entries:
        for t, pp in enumerate(p):
            ok, ratio, text = R.quantile_check(mu[:, e], var[:, e], pp, out[e, t])
            worst = max(worst, ratio)
            assert ok, (label, e, pp, out[e, t], text)
    print('%s quantile: max backward excess / cdf bound = %.3g' % (label, worst))
    return out


def check_crps(eng, mu, var, y, entries, label, path=None):
    out = npy(eng.mixture_crps(eng.tensor(mu), eng.tensor(var), eng.tensor(y), path=path))
    assert out.shape == (mu.shape[1],)
    worst, where = 0.0, None
    for e in entries:
        exact, bound = R.crps_and_bound(mu[:, e], var[:, e], y[e])
        ratio = float(abs(R.mp.mpf(float(out[e])) - exact)) / bound
        if ratio > worst:
            worst, where = ratio, (e, out[e], float(exact))
    print('%s crps: max error / bound = %.3g at %s' % (label, worst, where))
    assert worst <= 1.0, (label, worst, where)
    return out


# (S, count, T, y shared by all entries?, entries checked exactly beyond the fixed ones)
SHAPES = [(1, 1000, 3, False, 12), (2, 65, 5, True, 6), (7, 63, 1, False, 10), (64, 64, 3, True, 0), (65, 1, 5, False, 0),
          (200, 65, 1, False, 0), (7, 1000, 5, True, 4)]


@pytest.mark.parametrize('S,count,T,shared,k', SHAPES)
def test_cdf_sf_logpdf(eng, S, count, T, shared, k):
    mu, var = mixtures(S, count, seed=S * 1000 + count)
    y = thresholds(mu, var, T, seed=3)
    if shared:
        y = y[0]
    entries = chosen(count, k) if S < 64 else few(count)
    for what in ('cdf', 'sf', 'logpdf'):
        check_eval(eng, what, mu, var, y, entries, 'S=%d count=%d T=%d' % (S, count, T))


@pytest.mark.parametrize('S,count,T,k', [(1, 1000, 5, 10), (2, 65, 3, 6), (7, 63, 1, 8), (64, 64, 5, 0), (65, 1, 3, 0),
                                           (200, 65, 1, 0), (7, 1000, 3, 4)])
def test_quantile(eng, S, count, T, k):
    mu, var = mixtures(S, count, seed=S * 1000 + count + 1)
    p = {1: np.array([0.3]), 3: np.array([0.025, 0.5, 0.975]), 5: P5}[T]
    entries = chosen(count, k) if S < 64 else few(count)
    out = check_quantile(eng, mu, var, p, entries, 'S=%d count=%d T=%d' % (S, count, T))
    assert np.all(np.diff(out, axis=1) >= 0)
    if S == 1:   # one component: mu + zp sigma to rounding (an fma of the correctly rounded sqrt)
        want = mu[0][:, None] + ndtri(p)[None, :] * np.sqrt(var[0])[:, None]
        ulp = np.spacing(np.maximum(np.abs(mu[0])[:, None], np.abs(want - mu[0][:, None])))
        assert np.all(np.abs(out - want) <= 4 * ulp)
    if S == 2:   # against the bisection of the exact cdf, at one entry
        for t, pp in enumerate(p):
            exact = R.quantile(mu[:, 0], var[:, 0], pp)
            f = R._exact_pdf(mu[:, 0], var[:, 0], exact)
            allowed = R.quantile_delta(mu[:, 0], out[0, t]) + R.cdf_bound(mu[:, 0], var[:, 0], out[0, t]) / f
            assert abs(R.mp.mpf(float(out[0, t])) - exact) <= allowed, (pp, out[0, t], exact)


@pytest.mark.parametrize('S,count,k', [(1, 1000, 10), (2, 65, 6), (7, 63, 8), (64, 64, 0), (65, 1, 0), (200, 65, 0), (7, 1000, 4)])
def test_crps(eng, S, count, k):
    mu, var = mixtures(S, count, seed=S * 1000 + count + 2)
    y = thresholds(mu, var, 1, seed=5)[:, 0]
    entries = chosen(count, k) if S < 64 else few(count)[-2:] if S < 200 else few(count)[-1:]   # (the pair sum is S^2 / 2 terms in mpmath)
    check_crps(eng, mu, var, y, entries, 'S=%d count=%d' % (S, count))


# ----------------------------------------------------------------------------------------------------------- the hard contents
def test_zero_variance_components(eng):
    """Point masses: one among positive components, all of them, and y exactly on one (the step is right-continuous)."""
    mu, var = mixtures(5, 70, seed=12)
    var[2] = 0.0                                   # one point mass in every entry
    var[:, 64:] = 0.0                              # entries 64 .. 69: point masses only
    var[0, 3] = -1e-300                            # (a non-positive variance of either sign)
    y = thresholds(mu, var, 3, seed=13)
    y[:, 1] = mu[2]                                # exactly on the point mass
    y[66, 2] = mu[:, 66].max()
    entries = list(range(0, 70, 7)) + [3, 64, 65, 66, 69]
    out = {w: check_eval(eng, w, mu, var, y, entries, 'point masses') for w in ('cdf', 'sf', 'logpdf')}
    assert np.all(out['logpdf'][64:] == -np.inf) and np.all(np.isfinite(out['logpdf'][:64]))
    assert out['cdf'][66, 2] == 1.0 and out['sf'][66, 2] == 0.0
    on = (mu[:, 64:] <= mu[2, 64:][None]).mean(0)  # all point masses: the cdf at one of them counts it
    off = (mu[:, 64:] > mu[2, 64:][None]).mean(0)
    assert np.array_equal(out['cdf'][64:, 1], on) and np.array_equal(out['sf'][64:, 1], off)
    q = check_quantile(eng, mu, var, np.array([0.05, 0.3, 0.5, 0.9]), entries, 'point masses')
    gap = np.abs(q[64:, None, :] - mu[:, 64:].T[:, :, None]).min(1)     # a mixture of point masses: every quantile is one of them
    assert np.all(gap <= 4 * R.EPS * np.abs(mu[:, 64:]).max(0)[:, None])
    yc = y[:, 0].copy()
    yc[5] = mu[2, 5]
    check_crps(eng, mu, var, yc, entries, 'point masses')


@pytest.mark.parametrize('S', [2, 7, 64, 200])
def test_identical_components_give_the_one_gaussian_quantile(eng, S):
    rng = np.random.default_rng(S)
    count = 65
    m, v = 3.0 * rng.normal(size=count), np.exp(rng.normal(size=count))
    mu, var = np.tile(m, (S, 1)), np.tile(v, (S, 1))
    out, capped = eng.mixture_quantile(eng.tensor(mu), eng.tensor(var), P5)
    out = npy(out)
    zs = ndtri(P5)[None, :] * np.sqrt(v)[:, None]
    want = m[:, None] + zs
    ulp = np.spacing(np.maximum(np.abs(m)[:, None], np.abs(zs)))   # (the rounding of the sum's larger operand: 4 ulp of it)
    print('identical components, S=%d: max |q - (mu + zp sigma)| / ulp = %.3g' % (S, (np.abs(out - want) / ulp).max()))
    assert capped == 0 and np.all(np.abs(out - want) <= 4 * ulp)


def test_two_modes_forty_sigma_apart(eng):
    """p in the gap (with two equal modes 1/2 is the plateau's own level), in each mode and in either far tail."""
    sig = np.array([1.0, 0.25, 7.0])
    mu = np.stack([np.array([0.0, -3.0, 100.0]), np.array([0.0, -3.0, 100.0]) + 40 * sig])
    var = np.stack([sig ** 2, sig ** 2])
    p = np.array([1e-12, 0.1, 0.25, 0.4999, 0.5, 0.5001, 0.75, 0.9, 1 - 1e-12])
    out = check_quantile(eng, mu, var, p, range(3), 'two modes')
    assert np.all(out[:, :4] < mu[0][:, None] + 10 * sig[:, None]) and np.all(out[:, 5:] > mu[1][:, None] - 10 * sig[:, None])
    y = np.stack([mu[0] + 20 * sig, mu[0] + 0.3 * sig, mu[1] - 1.5 * sig], 1)
    for what in ('cdf', 'sf', 'logpdf'):
        check_eval(eng, what, mu, var, y, range(3), 'two modes')
    check_crps(eng, mu, var, y[:, 0], range(3), 'two modes')


@pytest.mark.parametrize('S', [1, 3])
def test_far_tails_keep_their_relative_accuracy(eng, S):
    """|z| up to 35: the cdf below and the upper tail above stay relatively accurate (sf is not 1 - cdf)."""
    z = np.concatenate((np.linspace(-35, 35, 29), [-35.0, -30.0, 30.0, 35.0]))
    rng = np.random.default_rng(2)
    mu = np.tile(rng.normal(size=(1, 1)), (S, len(z))) + (0 if S == 1 else 1e-3 * rng.normal(size=(S, len(z))))
    var = np.full((S, len(z)), 2.3)
    y = (mu[0] + z * np.sqrt(2.3))[:, None]
    cdf = check_eval(eng, 'cdf', mu, var, y, range(len(z)), 'far tails S=%d' % S)
    sf = check_eval(eng, 'sf', mu, var, y, range(len(z)), 'far tails S=%d' % S)
    check_eval(eng, 'logpdf', mu, var, y, range(len(z)), 'far tails S=%d' % S)
    assert 0 < sf[-1, 0] < 1e-260 and 0 < cdf[-4, 0] < 1e-260
    rel = abs(R.mp.mpf(float(sf[-2, 0])) - R.sf(mu[:, -2], var[:, -2], y[-2, 0])) / R.sf(mu[:, -2], var[:, -2], y[-2, 0])
    assert rel < 1e-12, float(rel)     # (z = 30: 1 - cdf would have returned 0)


def test_large_means_and_scales_across_sixteen_decades(eng):
    rng = np.random.default_rng(21)
    S, count = 7, 40
    mu = np.concatenate((1e8 + rng.normal(size=(S, count // 2)), rng.normal(size=(S, count // 2))), 1)
    var = np.concatenate((np.exp(0.3 * rng.normal(size=(S, count // 2))),          # mu ~ 1e8, sigma ~ 1
                          10.0 ** rng.uniform(-16, 16, size=(S, count // 2))), 1)  # sigma from 1e-8 to 1e8 within one mixture
    y = thresholds(mu, var, 3, seed=22)
    y[count // 2:, 2] = rng.normal(size=count // 2)
    entries = range(0, count, 3)
    for what in ('cdf', 'sf', 'logpdf'):
        check_eval(eng, what, mu, var, y, entries, 'large mu / wide sigma')
    check_quantile(eng, mu, var, P5, entries, 'large mu / wide sigma')
    check_crps(eng, mu, var, y[:, 2], entries, 'large mu / wide sigma')


# ----------------------------------------------------------------------------------------------------------------- bit equality
def test_slices_reproduce_the_call_bit_for_bit(eng):
    import torch
    mu, var = mixtures(7, 1000, seed=31)
    var[3, ::17] = 0.0
    y = thresholds(mu, var, 3, seed=32)
    mud, vard, yd = eng.tensor(mu), eng.tensor(var), eng.tensor(y)
    p = np.array([0.025, 0.5, 0.975])
    whole = [eng.mixture_eval(w, mud, vard, yd) for w in ('cdf', 'sf', 'logpdf')]
    whole += [eng.mixture_eval('cdf', mud, vard, yd[0].contiguous()), eng.mixture_quantile(mud, vard, p)[0], eng.mixture_crps(mud, vard, yd[:, 0].contiguous())]
    for lo, hi in ((0, 1), (1, 65), (65, 1000)):
        ms, vs, ys = mud[:, lo:hi].contiguous(), vard[:, lo:hi].contiguous(), yd[lo:hi].contiguous()
        part = [eng.mixture_eval(w, ms, vs, ys) for w in ('cdf', 'sf', 'logpdf')]
        part += [eng.mixture_eval('cdf', ms, vs, yd[0].contiguous()), eng.mixture_quantile(ms, vs, p)[0], eng.mixture_crps(ms, vs, ys[:, 0].contiguous())]
        for a, b in zip(whole, part):
            assert torch.equal(a[lo:hi], b), (lo, hi)


@pytest.mark.parametrize('S', [7, 65])
def test_lds_and_global_kernels_agree(eng, S):
    mu, var = mixtures(S, 130, seed=41)
    var[1, ::9] = 0.0
    y = thresholds(mu, var, 1, seed=42)[:, 0]
    mud, vard, yd = eng.tensor(mu), eng.tensor(var), eng.tensor(y)
    ql, cl = eng.mixture_quantile(mud, vard, P5, path='lds')
    qg, cg = eng.mixture_quantile(mud, vard, P5, path='global')
    assert cl == 0 and cg == 0
    np.testing.assert_allclose(npy(ql), npy(qg), rtol=1e-13, atol=0)
    np.testing.assert_allclose(npy(eng.mixture_crps(mud, vard, yd, path='lds')), npy(eng.mixture_crps(mud, vard, yd, path='global')),
                               rtol=1e-13, atol=0)


def test_refusals(eng):
    from dgp_amd.ops import DgpAmdError
    mu, var = (eng.tensor(a) for a in mixtures(3, 10, seed=51))
    for bad in (np.array([0.0]), np.array([0.5, 1.0]), np.array([np.nan]), np.array([-0.1])):
        with pytest.raises(ValueError):
            eng.mixture_quantile(mu, var, bad)
    with pytest.raises(ValueError):
        eng.mixture_eval('cdf', mu, var[:2], eng.tensor(np.zeros(1)))
    with pytest.raises(ValueError):
        eng.mixture_eval('cdf', mu, var, eng.tensor(np.zeros((9, 2))))
    with pytest.raises(ValueError):
        eng.mixture_crps(mu, var, eng.tensor(np.zeros(9)))
    big = eng.tensor(np.zeros((200, 4)))
    with pytest.raises(DgpAmdError):
        eng.mixture_crps(big, big + 1.0, eng.tensor(np.zeros(4)), path='lds')     # 200 components do not fit the LDS of a CU
    out, capped = eng.mixture_quantile(eng.tensor(np.full((2, 3), np.nan)), eng.tensor(np.ones((2, 3))), np.array([0.5]))
    assert np.all(np.isnan(npy(out)))           # (NaN components: passed through, never looped on; PredictiveMixture refuses them)
    many = np.linspace(0.01, 0.99, 70)          # more probabilities than one launch takes: split, same results
    q, _ = eng.mixture_quantile(mu, var, many)
    q1, _ = eng.mixture_quantile(mu, var, many[33:34])
    assert q.shape == (10, 70) and np.array_equal(npy(q)[:, 33], npy(q1)[:, 0])
