"""The host log-densities of dgp_amd/likelihood_class.py (llik and pllik of Poisson, NegBin, ZIP, ZINB and of Categorical with its
four links) against exact values (tests/lik_ref.py: mpmath from the definitions), on the grids tests/test_gpu_lik.py runs on
the device, under the same bound; and the measurement of the bound's constant (no GPU)."""
import math

import numpy as np
import pytest

import lik_ref as R


def _node(kind, K=None):
    from dgp_amd import Poisson, NegBin, ZIP, ZINB, Categorical
    if kind in ('Poisson', 'NegBin', 'ZIP', 'ZINB'):
        return {'Poisson': Poisson, 'NegBin': NegBin, 'ZIP': ZIP, 'ZINB': ZINB}[kind]()
    return Categorical(num_classes=2 if kind in ('logit', 'probit') else K, link=kind, robustmax_eps=R.EPS)


def _host_values(kind, y, F, K=None):
    """(llik of every row as a one-observation node, pllik of every row as one quadrature node): two (R,) arrays."""
    node = _node(kind, K)
    ll = np.empty(len(F))
    with np.errstate(all='ignore'):
        for r in range(len(F)):
            node.input, node.output = F[r:r + 1], np.array([[y]])
            ll[r] = float(node.llik())
        pl = np.asarray(node.pllik(np.full((len(F), 1, 1), y), F[:, None, :]), dtype=float).reshape(len(F))
    return ll, pl


def _cases(kind, classes=(2, 3, 4, 64)):
    """(label, y, K, F, ex, lo, T) of every grid the kind is run on."""
    if kind in R.NCOL:
        return [('y=%g' % y, y, None) + R.point_reference(kind, y) for y in R.point_ys(kind)]
    return [('K=%d y=%d' % (K, y), float(y), K) + R.class_reference(kind, K, y) for K in classes for y in R.class_ys(K)]


def _worst(got, ex, lo, T):
    """Largest |got - exact| / (2^-53 T + 2^-1074) over the rows, exact = ex + lo; every row must be finite."""
    assert np.all(np.isfinite(ex)) and np.all(np.isfinite(got)), (got[~np.isfinite(got)], ex[~np.isfinite(ex)])
    return float(np.max(np.abs((got - ex) - lo) / (R.U * T + R.TINY)))


@pytest.mark.parametrize('kind', R.KINDS)
def test_stable64_within_measured_c(kind):
    """Where c comes from: the stable float64 form against exact values on every input of the point tests and, for the two
    kinds that are summed, on the 300 pairs of the sum tests.  It stays within C_MEASURED (the measured value rounded up to two
    decimals), and the asserted C is four times that."""
    worst = 0.0
    for label, y, K, F, ex, lo, T in _cases(kind):
        got = R.stable64(kind, np.full(len(F), y), F, classes=K, eps=R.EPS)
        worst = max(worst, _worst(got, ex, lo, T))
    if kind in ('Poisson', 'ZINB'):
        L, hi, lo, T = R.sum_reference(kind)
        for v, y in enumerate(R.SUM_Y):
            worst = max(worst, _worst(R.stable64(kind, np.full(30, y), L), hi[v], lo[v], T[v]))
    print('PARITY stable64 %-9s measured c = %.3f  recorded %.2f  asserted C = %.1f' % (kind, worst, R.C_MEASURED[kind], R.C[kind]))
    assert worst <= R.C_MEASURED[kind]
    assert R.C[kind] == 4.0 * R.C_MEASURED[kind]


@pytest.mark.parametrize('kind', R.KINDS)
def test_host_log_densities_against_exact(kind):
    """llik() and pllik() of the host classes within C 2^-53 T of the exact value at every grid row: the wild latents in every
    pairing, counts up to 10^6, the switch points of logaddexp, of the probit tail and of the lgamma difference.  (Two classes
    are logit / probit on the host: the two-class softmax and robustmax grids are the device's alone.)"""
    worst = 0.0
    for label, y, K, F, ex, lo, T in _cases(kind, (3, 4, 64)):
        ll, pl = _host_values(kind, y, F, K)
        for name, got in (('llik', ll), ('pllik', pl)):
            w = _worst(got, ex, lo, T)
            assert w <= R.C[kind], (kind, name, label, w)
            worst = max(worst, w)
    print('PARITY host %-9s worst error / (2^-53 T) = %.3f of C = %.1f' % (kind, worst, R.C[kind]))


def test_host_non_finite_inputs_keep_their_class():
    """Where the definition is no finite double -- a NaN latent, e^f beyond the double range -- the host gives the same class."""
    for kind, y, row, cls in R.NONFINITE:
        ex = R.to_float(R.exact(kind, y, row))
        assert R.same_class(ex, cls), (kind, y, row, ex)
        ll, pl = _host_values(kind, y, np.array([row]))
        assert R.same_class(ll[0], cls) and R.same_class(pl[0], cls), (kind, y, row, ll, pl)
    for K in (3, 4, 64):
        F, winners = R.nan_class_rows(K)
        for y in R.class_ys(K):
            ll, pl = _host_values('robustmax', float(y), F, K)
            want = np.where(np.asarray(winners) == y, math.log1p(-R.EPS), math.log(R.EPS / (K - 1)))
            assert np.allclose(ll, want, rtol=4 * R.U, atol=0) and np.allclose(pl, want, rtol=4 * R.U, atol=0)
            ex = np.array([R.to_float(R.exact('robustmax', y, r, classes=K, eps=R.EPS)) for r in F])
            assert np.allclose(ex, want, rtol=4 * R.U, atol=0)
            sm, _ = _host_values('softmax', float(y), F, K)
            assert np.all(np.isnan(sm))


def test_the_table_of_defects():
    """The inputs at which the earlier expressions were wrong (NegBin above the rising sum with a huge size, log1p(-expit(f)),
    the probit series at its old switch): the exact values, and the host within the bound of each."""
    rows = [('NegBin', 100.0, [4.5, -37.0], -3.757), ('NegBin', 100.0, [4.5, -20.0], -3.7565069),
            ('ZIP', 2.0, [1.0, 30.0], -31.41143), ('ZIP', 2.0, [1.0, 37.0], -38.41), ('probit', 1.0, [-20.0 - 1e-7], -203.917)]
    for kind, y, row, quoted in rows:
        ex = R.exact(kind, y, row)
        assert abs(float(ex) - quoted) <= 6e-3 * max(1.0, abs(quoted) / 40), (kind, row, float(ex))
        hi, lo = R.split(ex)
        F = np.array([row])
        T = R.terms(kind, [y], F, ex=[hi])
        ll, pl = _host_values(kind, y, F)
        assert abs((ll[0] - hi) - lo) <= R.point_bound(kind, T[0]) and abs((pl[0] - hi) - lo) <= R.point_bound(kind, T[0]), (kind, row, ll, hi)


def test_sum_cases_are_what_they_claim():
    """The replicate map is a permutation of the rows with repeats and not monotone; blocks differ; 300 distinct pairs."""
    L, hi, lo, T = R.sum_reference('ZINB')
    assert len({tuple(r) for r in L}) == 30 and hi.shape == (10, 30) and len(set(R.SUM_Y)) == 10
    c = R.sum_case('ZINB', 8193, 3)
    assert sorted(c['rep'][:300].tolist()) == list(range(300)) and np.any(np.diff(c['rep']) < 0) and len(c['rep']) == 8193
    assert not np.array_equal(c['FP'][0], c['FP'][1]) and len(set(c['want'].tolist())) == 3
    assert np.all(np.isfinite(c['want'])) and np.all(c['bound'] < 1e-9 * np.abs(c['want']))
    assert R.sum_case('Poisson', 8193, 1, mapped=False)['FP'].shape == (1, 8193, 1)
