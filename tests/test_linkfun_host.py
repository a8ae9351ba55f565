"""tests/linkfun_ref.py checked without a GPU: the exact Matern-2.5 linked-GP factors against the defining integral and their
invariances, the committed fixture against a regenerated subsample, the float64 restatement of csrc/linkfun.hpp's algorithm
against the exact values per v/l^2 bucket (the E_b the GPU tests scale their bounds by, held to the caps of BUCKET_CAPS), and
the oracle's restatement of the reference expression, which is NOT the judge from v/l^2 = 4 on."""
import numpy as np
import pytest

import linkfun_ref as R

mp = pytest.importorskip('mpmath')


@pytest.fixture(scope='module')
def fx():
    return R.load()


def quad_cases():
    """31 cases by index: one or two per v/l^2 of the case set, moving through lengthscales, means and pairs."""
    args, ratio = R.cases()
    per = 9 * 21
    idx = [r * per + (37 * r + 5) % per for r in range(len(R.RATIOS))] + [r * per + (53 * r + 101) % per for r in range(11, 21)]
    return args[idx], ratio[idx]


def test_closed_form_equals_the_defining_integral():
    """exact_J against mpmath.quad of k(x1 - z) k(x2 - z) N(z; m, v), to 1e-30 relative, over the whole range of v/l^2 (a tail
    written as 1 + erf loses 4.3 v/l^2 digits of the DPS = 120 carried and fails here from v/l^2 ~ 25 on)."""
    args, ratio = quad_cases()
    assert ratio.min() <= 1e-12 and ratio.max() >= 1600 and len(set(ratio)) == len(set(R.RATIOS))
    worst = 0
    for (x1, x2, m, v, l) in args:
        e = R.exact_J(x1, x2, m, v, l)
        assert e > 0
        err = abs(R.quad_J(x1, x2, m, v, l, scale=e) - 1)
        worst = max(worst, err)
        assert err <= mp.mpf(10) ** -30, (x1, x2, m, v, l, mp.nstr(err, 5))
    print('largest relative difference from quad: %s' % mp.nstr(worst, 3))


def test_exact_I_equals_its_integral():
    for (x, m, v, l) in ((0.3, 0.1, 1.0, 1.0), (-40.5, -40.0, 9.0 * 1600, 3.0), (1.5, 1.5, 0.0025 * 100, 0.05), (3.0, 0.0, 1e-6, 1.0)):
        with mp.workdps(50):
            e = R.exact_I(x, m, v, l)
            x, m, v, l = (mp.mpf(t) for t in (x, m, v, l))
            k = lambda d: (1 + mp.sqrt(5) * abs(d) / l + 5 * d * d / (3 * l * l)) * mp.exp(-mp.sqrt(5) * abs(d) / l)
            sd = mp.sqrt(v)
            f = lambda z: k(x - z) * mp.exp(-(z - m) ** 2 / (2 * mp.mpf(v))) / (mp.sqrt(2 * mp.pi * v) * e)
            cuts = sorted({x, m} | {m + s * sd for s in (-40, -12, -4, 4, 12, 40)} | {x + s * l for s in (-8, -1, 1, 8)})
            assert abs(mp.quad(f, [-mp.inf] + cuts + [mp.inf], maxdegree=10) - 1) <= mp.mpf(10) ** -30, (x, m, v, l)


def test_symmetry_and_invariance():
    """J(x1, x2) = J(x2, x1), and J(x1, x2, m, v, l) = J((x1 - m)/l, (x2 - m)/l, 0, v/l^2, 1) (dyadic numbers: the float
    normalisation is exact)."""
    m, l = 1.5, 0.5
    for R_ in (2.0 ** -30, 0.125, 1.0, 4.0, 32.0, 512.0):
        for (u1, u2) in ((0.0, 0.0), (0.25, -2.0), (-8.0, -8.0), (2.0, 64.0), (-0.5, 2.0 ** -20)):
            x1, x2, v = m + u1 * l, m + u2 * l, R_ * l * l
            a, b, c = R.exact_J(x1, x2, m, v, l), R.exact_J(x2, x1, m, v, l), R.exact_J(u1, u2, 0.0, R_, 1.0)
            assert a == b
            assert abs(a - c) <= a * mp.mpf(10) ** -100, (R_, u1, u2)
            i1, i2 = R.exact_I(x1, m, v, l), R.exact_I(u1, 0.0, R_, 1.0)
            assert abs(i1 - i2) <= i1 * mp.mpf(10) ** -100


def test_limits():
    """Jd -> Jd0 as x2 -> x1 (linearly in the distance), and J -> k(x1 - m) k(x2 - m), I -> k(x - m) as v -> 0 (the correction
    is O(v / l^2))."""
    for (x, m, v, l) in ((0.3, 0.0, 1.0, 1.0), (1.4, 1.5, 0.25, 0.05), (-38.0, -40.0, 900.0, 3.0)):
        j0 = R.exact_J(x, x, m, v, l)
        for eps in (1e-6, 1e-9, 1e-12):
            assert abs(R.exact_J(x, x + eps * l, m, v, l) - j0) <= 4 * eps * j0
    for (x1, x2, m, l) in ((0.3, -0.2, 0.0, 1.0), (1.5, 1.6, 1.5, 0.05), (-10.0, -70.0, -40.0, 3.0)):
        with mp.workdps(R.DPS):
            k = lambda x: R._kpoint((mp.mpf(x) - mp.mpf(m)) / mp.mpf(l))
            kk, k1 = k(x1) * k(x2), k(x1)
        for w in (1e-20, 1e-30):
            assert abs(R.exact_J(x1, x2, m, w * l * l, l) - kk) <= 20 * w * kk
            assert abs(R.exact_I(x1, m, w * l * l, l) - k1) <= 20 * w * k1
        assert R.exact_J(x1, x2, m, 0.0, l) == kk


def test_case_set(fx):
    args, ratio = R.cases()
    assert 3900 <= len(args) <= 4300
    assert np.array_equal(args, fx['args']) and np.array_equal(ratio, fx['ratio'])
    X1, X2, m, v, l = args.T
    u1, u2 = (X1 - m) / l, (X2 - m) / l
    assert (X1 == X2).sum() >= 150 and ((X1 != X2) & (np.abs(u1 - u2) < 2e-7)).sum() >= 300          # equal points, points 1e-7 apart
    assert ((u1 < 0) & (u2 > 0)).sum() >= 300 and ((X1 == m) != (X2 == m)).sum() >= 150              # straddling m, one point on m
    assert (v == 0).sum() >= 30 and (v == 1e-300).sum() >= 30 and (np.abs(u1) > 9e4).sum() >= 50


def test_fixture_is_the_exact_values(fx):
    """200 cases by index, regenerated and compared bit for bit (the whole fixture: python -m tests.linkfun_ref)."""
    n = len(fx['args'])
    idx = (np.arange(200) * 7919 + 13) % n
    ei, ej, e0 = R.exact_rows(fx['args'], idx)
    assert np.array_equal(ei, fx['exact_i'][idx]) and np.array_equal(ej, fx['exact_j'][idx]) and np.array_equal(e0, fx['exact_j0'][idx])
    for k in ('exact_i', 'exact_j', 'exact_j0'):
        assert np.all(np.isfinite(fx[k])) and fx[k].min() >= 0.0 and fx[k].max() <= 1.0


def test_restatement_error_per_bucket(fx):
    """E_b of the float64 restatement of csrc/linkfun.hpp on the full case set: below the caps, and what the fixture carries
    for the GPU tests.  Cases with exact < 1e-280 are held to |got| <= 1e-279 (relative_error returns inf otherwise)."""
    E_b, table = R.measure_E_b(fx['args'], fx['ratio'], fx)
    for fn in R.FNS:
        print('%-6s' % fn, ' '.join('%.1e' % e for e in table[fn]))
    print('E_b   ', ' '.join('%.1e' % e for e in E_b), ' caps', R.BUCKET_CAPS)
    assert np.all(np.isfinite(E_b)) and np.all(E_b <= np.array(R.BUCKET_CAPS)), E_b
    assert np.allclose(E_b, fx['E_b'], rtol=0.25)           # (scipy's erfc / erfcx may differ by an ulp between versions)
    b = R.bucket_of(fx['ratio'])
    assert np.all(np.bincount(b, minlength=len(R.BUCKET_EDGES)) >= 180)


def test_the_oracle_expression_is_not_the_judge_from_4_on(fx):
    """The oracle's float64 Jd (the reference's expression) against the exact values: off by more than 1e-3 (or not
    finite) at every v/l^2 >= 4 of the case set.  (Up to 0.1 the figure printed is its absolute error: its polynomials are expanded
    about 0 and not about m, and with m = -40, l = 0.05 they cancel like (m/l)^4 -- 1.5e-3 at any v.)"""
    from oracle import dgp_oracle as O
    args, ratio, ex = fx['args'], fx['ratio'], fx['exact_j']
    worst = {}
    with np.errstate(all='ignore'):
        for k in np.where((ratio >= 1e-12) & (np.abs((args[:, 0] - args[:, 2]) / args[:, 4]) < 9e4) & (np.abs((args[:, 1] - args[:, 2]) / args[:, 4]) < 9e4))[0]:
            X1, X2, m, v, l = args[k]
            got = float(np.asarray(O.Jd(np.array([X1]), np.array([X2]), m, v, l)).reshape(-1)[0])
            if not np.isfinite(got):
                err = np.inf
            else:
                err = abs(got - ex[k]) / (ex[k] if ratio[k] > 0.1 else 1.0)
            worst[ratio[k]] = max(worst.get(ratio[k], 0.0), err)
    print({r: '%.1e' % w for r, w in sorted(worst.items())})
    for r, w in worst.items():
        if r >= 4.0:
            assert w > 1e-3, (r, w)
