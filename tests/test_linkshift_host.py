"""tests/linkshift_ref.py on the host: the shifts are exact, the long-double reference does not see them, it agrees with the
oracle at offset 0, and the bound it offers the device discriminates -- float64 restatements of the pair exponent in the
difference-first orders keep it at every offset, the expanded order breaks it from offset 2^6 on, on every shape of the
GPU test (tests/test_gpu_linkgp_shift.py)."""
import numpy as np
import pytest

import linkshift_ref as R
from linkshift_ref import loo_drop, seed_of

CASES = [(n, Dw, Dz) for n in R.SIZES for (Dw, Dz) in R.SHAPES]


_cache = {}


def case_of(n, Dw, Dz):
    """(problem, exact) of one shape, computed once."""
    key = (n, Dw, Dz)
    if key not in _cache:
        p = R.problem('sexp', n, Dw, Dz, seed_of(n, Dw, Dz))
        _cache[key] = (p, R.exact_sexp(p))
    return _cache[key]


def close(a, b, rtol, atol):
    np.testing.assert_allclose(np.asarray(a, float), np.asarray(b, float), rtol=rtol, atol=atol)


@pytest.mark.parametrize('n,Dw,Dz', CASES)
def test_generator_lies_on_its_grids(n, Dw, Dz):
    p, _ = case_of(n, Dw, Dz)
    for a, step, lo, hi in ((p['W0'], 1024, 0.0, 1.0), (p['Wg0'], 1024, 0.0, 1.0), (p['m0'], 4096, -0.2, 1.2), (p['z0'], 1024, 0.0, 1.0)):
        assert np.array_equal(a * step, np.round(a * step)) and np.all(a >= lo) and np.all(a <= hi)
    assert np.linalg.cond(p['Rinv']) <= 1e4
    assert not p['v'][0].any() and p['v'][1, Dw - 1] == 0.0 and not p['v'][-1, :Dw // 2].any()
    assert np.all((p['v'] == 0.0) | ((p['v'] >= 1e-5) & (p['v'] <= 1e-1)))


@pytest.mark.parametrize('n,Dw,Dz', CASES)
def test_reference_is_the_oracle_at_offset_0(n, Dw, Dz):
    """exact_sexp against O.link_gp_predict (oracle.IJ's order) at the suite's linked-GP tolerances."""
    from oracle import dgp_oracle as O
    p, ex = case_of(n, Dw, Dz)
    mr, vr = O.link_gp_predict(p['m0'], p['v'], p['z0'] if Dz else None, p['W0'], p['Wg0'] if Dz else None, p['Rinv'], p['ry'],
                               p['scale'], p['length'], p['nugget'], 'sexp')
    close(ex['mean'], mr, rtol=1e-8, atol=1e-10)
    close(ex['var'], vr, rtol=1e-6, atol=1e-8)


@pytest.mark.parametrize('n,Dw,Dz', [(65, 3, 2), (130, 15, 0)])
def test_leave_one_out_reference_is_the_refit(n, Dw, Dz):
    """The leave-one-out exact values (long-double downdate of the given float64 statistics, what the device is asked
    for) against the refit on the other n - 1 points -- in long double (loo_refit) and by the oracle -- at the suite's
    tolerances; the float64 statistics carry cond(R) eps ~ 1e-12, which is why the sharp bound is taken on the downdate."""
    from oracle import dgp_oracle as O
    p, _ = case_of(n, Dw, Dz)
    drop = loo_drop(n)
    ex = R.exact_sexp(p, drop=drop)
    tests = [0, 1, 2, 3, R.M_TEST - 1]
    mr, vr = R.loo_refit(p, drop, tests)
    close(ex['mean'][tests], mr, rtol=1e-8, atol=1e-10)
    close(ex['var'][tests], vr, rtol=1e-6, atol=1e-8)
    X0 = np.concatenate((p['W0'], p['Wg0']), 1)
    for t in tests:
        keep = np.delete(np.arange(n), drop[t])
        s2 = O.compute_stats(X0[keep], p['y'][keep], p['length'], p['nugget'], 'sexp', Dw)
        mo, vo = O.link_gp_predict(p['m0'][t:t + 1], p['v'][t:t + 1], p['z0'][t:t + 1] if Dz else None, p['W0'][keep],
                                   p['Wg0'][keep] if Dz else None, s2['Rinv'], s2['Rinv_y'], p['scale'], p['length'], p['nugget'], 'sexp')
        close(ex['mean'][t], mo[0], rtol=1e-8, atol=1e-10)
        close(ex['var'][t], vo[0], rtol=1e-6, atol=1e-8)


@pytest.mark.parametrize('n,Dw,Dz', R.MATERN_EXACT_CASES)
def test_recorded_matern_reference_is_the_oracle_on_the_integral(n, Dw, Dz):
    """The recorded exact Matern predictions (tests/golden/linkshift_matern.npz) against O.link_gp_predict with its factors on
    the integral (linkfun_ref.oracle_on_the_integral) at the suite's tolerances; leave-one-out at the first four test points
    against the same oracle with the statistics refitted on the other n - 1 points."""
    import linkfun_ref
    from oracle import dgp_oracle as O
    p, dense, loo = R.matern_problem(n, Dw, Dz)
    z, Wg = (p['z0'], p['Wg0']) if Dz else (None, None)
    with linkfun_ref.oracle_on_the_integral(O):
        mr, vr = O.link_gp_predict(p['m0'], p['v'], z, p['W0'], Wg, p['Rinv'], p['ry'], p['scale'], p['length'], p['nugget'], 'matern2.5')
    close(dense['mean'], mr, rtol=1e-8, atol=1e-10)
    close(dense['var'], vr, rtol=1e-6, atol=1e-8)
    assert np.all(dense['A'] > 0) and np.all(dense['B'] > 0) and np.all(R.matern_rho(p) < 1e-8)
    drop = loo_drop(n)
    X0 = np.concatenate((p['W0'], p['Wg0']), 1)
    for t in range(4):
        keep = np.delete(np.arange(n), drop[t])
        s2 = O.compute_stats(X0[keep], p['y'][keep], p['length'], p['nugget'], 'matern2.5', Dw)
        with linkfun_ref.oracle_on_the_integral(O):
            mo, vo = O.link_gp_predict(p['m0'][t:t + 1], p['v'][t:t + 1], None if z is None else z[t:t + 1], p['W0'][keep],
                                       None if Wg is None else Wg[keep], s2['Rinv'], s2['Rinv_y'], p['scale'], p['length'], p['nugget'], 'matern2.5')
        close(loo['mean'][t], mo[0], rtol=1e-8, atol=1e-10)
        close(loo['var'][t], vo[0], rtol=1e-6, atol=1e-8)


@pytest.mark.parametrize('n,Dw,Dz', CASES)
def test_shifts_are_exact_and_the_reference_does_not_see_them(n, Dw, Dz):
    """shifted() asserts (W0 + off) - off == W0 (and m, Wg, z likewise) and the equality of every difference; the factors of
    the reference, recomputed from the shifted arrays, are then identical to the offset-0 ones at every shift."""
    p, _ = case_of(n, Dw, Dz)
    tests = [0, 1, 17, R.M_TEST - 1]
    at0 = [R.sexp_factors(p['W0'], p['Wg0'], p['m0'][t], p['v'][t], p['z0'][t], p['length']) for t in tests]
    for name, off in R.shifts(Dw + Dz).items():
        W, m, Wg, z = R.shifted(p, off)
        for t, ref in zip(tests, at0):
            got = R.sexp_factors(W, Wg, m[t], p['v'][t], z[t], p['length'])
            assert all(np.array_equal(g, r) for g, r in zip(got, ref)), (name, t)


@pytest.mark.parametrize('n,Dw,Dz', CASES)
def test_the_bound_separates_the_orders(n, Dw, Dz):
    """The variance with the pair exponent restated in float64 (everything else exact): 'direct' and 'centred' keep
    var_bound at every shift -- and return the same value at every shift --, 'expanded' breaks it at every shift of size
    >= 2^6.  This is what shows that the inputs and the constants of the GPU test can fail."""
    p, ex = case_of(n, Dw, Dz)
    bnd = R.var_bound(ex, p)
    rows, first = [], {}
    for name, off in R.shifts(Dw + Dz).items():
        W, m, Wg, z = R.shifted(p, off)
        got = {o: R.restated_var(o, p, W, Wg, m, z, ex['mean']) for o in ('expanded', 'direct', 'centred')}
        ratio = {o: R.worst_ratio(got[o], ex['var'], bnd) for o in got}
        rows.append('%-9s ' % name + ' '.join('%s %.2e' % (o, ratio[o]) for o in ratio))
        for o in ('direct', 'centred'):
            assert ratio[o] <= 1.0, (name, o, ratio[o])
            assert np.array_equal(got[o], first.setdefault(o, got[o])), (name, o)
        if R.shift_size(off) >= 2.0 ** 6:
            assert ratio['expanded'] > 1.0, (name, ratio['expanded'])
        else:
            assert ratio['expanded'] <= 1.0, (name, ratio['expanded'])
    print('\nn %d Dw %d Dz %d: worst error / bound\n  ' % (n, Dw, Dz) + '\n  '.join(rows))
